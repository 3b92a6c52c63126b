"""The HIP path against the independent float64 model of the detector, directly: the checker of tests/detector_cases.py
on a product context, not on the oracle (tests/test_detector_model.py does that, and shows that the checker notices each
wrong rule).  The parity suite says that the kernels equal the oracle; this file says that they follow the reference's
rules, also where kernels and oracle were written from one reading of them -- in the Hessian mode and in the
difference-of-Gaussians mode (the `dog:` cases), on single images and inside a batch of three (level-by-level launches,
24-row scan segments, copier delivery).

The checker reads every level, so it runs with keep_levels(True), which turns the LDS-resident forms off (level 0 in LDS,
top-level fusion).  After it the same input runs once more with keep_levels(False), the schedule users get, and the raw
list, the keypoints and the descriptors must be byte-equal to those the model has just judged.

Nothing of the model is cached between tests: every stage is computed from the session's own previous stage, so the
model's results belong to the session under test; only the images (detector_cases.cases) are shared.
"""
import pytest

import detector_cases as dc

pytestmark = pytest.mark.gpu

CASES = list(dc.cases())


def _judged(g, index, case):
    """The results the context holds now; a keypoint-list run has no raw list of its own."""
    keys, desc = g.fetch(index)
    raw = g.rawlist(index).tobytes() if case.keys is None else b""
    return raw, keys.tobytes(), desc.tobytes()


@pytest.mark.parametrize("name", CASES)
def test_hip_path_follows_the_model(gpu_ctx_factory, name):
    case = dc.cases()[name]
    g = gpu_ctx_factory(**case.kw)
    st = dc.check_against_model(g, case)
    print(name, st)
    dc.check_statistics(st, case)
    # the production schedule gives what the model has just judged
    stack, index = dc.case_input(case)
    kept = _judged(g, index, case)
    g.keep_levels(False)
    g.run(stack, fmt=case.fmt)
    if case.keys is not None:
        g.run_keypoints(case.keys, case.have_orientation)
    prod = _judged(g, index, case)
    assert len(kept[1]) > 0
    for what, a, b in zip(("raw list", "keypoints", "descriptors"), kept, prod):
        assert a == b, f"{what}: keep_levels(False) differs from the kept-levels run"
