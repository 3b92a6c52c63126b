"""The HIP path against the independent float64 model of the detector, directly: the checker of tests/detector_cases.py
on a product context, not on the oracle (tests/test_detector_model.py does that, and shows that the checker notices each
wrong rule).  The parity suite says that the kernels equal the oracle; this file says that they follow the reference's
rules, also where kernels and oracle were written from one reading of them.

Nothing of the model is cached between tests: every stage is computed from the session's own previous stage, so the
model's results belong to the session under test; only the images (detector_cases.cases) are shared.
"""
import pytest

import detector_cases as dc

pytestmark = pytest.mark.gpu

CASES = list(dc.cases())


@pytest.mark.parametrize("name", CASES)
def test_hip_path_follows_the_model(gpu_ctx_factory, name):
    case = dc.cases()[name]
    g = gpu_ctx_factory(**case.kw)
    st = dc.check_against_model(g, case)
    print(name, st)
    dc.check_statistics(st, case)
