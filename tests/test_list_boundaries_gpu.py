"""The list stages at their count-set seams on the HIP path: every case of list_cases.cases() -- the row scan on both sides of
32 768 list rows, a spill list longer than the placement grid covers, the top-K cut on and around the 4 096-entry chunk
edges, the feature scan over more than one pass of 16 384 keypoints and in chunks of which the last are empty --
(a) byte for byte against the CPU oracle (raw list, keypoints, descriptors, of every image of the batch), (b) against the
plain list model applied to the device's OWN untruncated list, with the reach of every case asserted from that list,
(c) once more through submit_host / wait (the throughput schedule, 24-row scan segments, copier delivery), same bytes;
then (d) one context through a large row-scan case, a top-K case, a 4 x 1 image and the large case again, byte-equal to fresh
contexts.  tests/test_list_boundaries.py holds the oracle to the model on the same cases and shows what each wrong version
of a rule would give.

Contexts: one per case and parameter set, closed after the case -- a fresh context has the planned capacities the cases are
stated for (the feature scan's chunk count follows the planned list capacity; the placement cases must not re-run).
"""
import hashlib
from contextlib import closing

import numpy as np
import pytest

import list_cases as L
from oracle_lib import OracleSession

pytestmark = pytest.mark.gpu

CASES = L.cases()


class _Runs:
    """Runs of one side: (input, parameters) -> [Result per image].  Untruncated runs are kept for the file (the cases of one
    input share them), of the truncating ones the last (the images of one batch are cases of their own)."""

    def __init__(self):
        self.full, self.last = {}, (None, None)

    def get(self, key, keep, make):
        if key in self.full:
            return self.full[key]
        if self.last[0] == key:
            return self.last[1]
        res = make()
        if keep:
            self.full[key] = res
        else:
            self.last = (key, res)
        return res


_ORACLE, _DEVICE = _Runs(), _Runs()


def _same(a, b, what):
    assert a.counts == b.counts, f"{what}: feature counts {a.counts} != {b.counts}"
    assert len(a.raw) == len(b.raw), f"{what}: list length {len(a.raw)} != {len(b.raw)}"
    assert a.raw.tobytes() == b.raw.tobytes(), f"{what}: detection list differs"
    assert a.keys.tobytes() == b.keys.tobytes(), f"{what}: keypoints differ"
    assert a.desc.tobytes() == b.desc.tobytes(), f"{what}: descriptors differ"


def _all(session, counts):
    return [L.result_of(session, counts, b) for b in range(len(counts))]


def device_runner(case, factory, regrown):
    imgs = case.image()
    digest = hashlib.md5(imgs.tobytes()).hexdigest()

    def oracle(kw):
        with closing(OracleSession(threads=16, keep_levels=False, **kw)) as o:
            return _all(o, o.run(imgs))

    def device(kw):
        g = factory(**kw)
        try:
            res = _all(g, g.run(imgs))
            g.submit_host(imgs)
            g.wait()
            again = _all(g, [g.count(b) for b in range(len(imgs))])
            for b in range(len(imgs)):
                _same(again[b], res[b], f"{case.name}: image {b} submitted against run")
            regrown.append(g.regrown())
        finally:
            g.close()
        return res

    def run(kw):
        key = (digest, imgs.shape, tuple(sorted(kw.items())))
        want = _ORACLE.get(key, kw == case.base, lambda: oracle(kw))
        got = _DEVICE.get(key, kw == case.base, lambda: device(kw))
        for b in range(len(imgs)):
            _same(got[b], want[b], f"{case.name}: image {b} against the oracle {kw}")
        return got[case.index]

    return run


@pytest.mark.parametrize("name", list(CASES))
def test_hip_path_at_the_list_seams(gpu_ctx_factory, name):
    case = CASES[name]
    regrown = []
    st = L.check_case(device_runner(case, gpu_ctx_factory, regrown), case)
    L.check_reach(st, case)
    if case.reach.get("spill"):
        assert not any(regrown), f"the batch ran again after an overflow ({regrown}): the planned capacity was to hold it"


def test_one_context_through_large_and_small_lists(gpu_ctx_factory):
    """Ticket, state and flag words of placement and top-K are cleared per batch: a context that goes from 43 008 list rows to
    a top-K cut in the second chunk of 8 192 entries, to a plane without a detection, and back gives the bytes of fresh
    contexts."""
    kw = dict(L.TIE_BASE, truncate_method=L.T["topk"], feature_count_threshold=5000)
    inputs = [L.mixed_strip(8192)[None], L.tie_strip(8192)[None], np.array([[[7, 200, 31, 90]]], dtype=np.uint8), L.mixed_strip(8192)[None]]
    fresh = []
    for imgs in inputs[:3]:
        f = gpu_ctx_factory(**kw)
        fresh.append(_all(f, f.run(imgs)))
        f.close()
    fresh.append(fresh[0])
    assert len(fresh[0][0].raw) > 3000 and len(fresh[1][0].raw) == 5000 and len(fresh[2][0].raw) == 0
    g = gpu_ctx_factory(**kw)
    for i, imgs in enumerate(inputs):
        _same(_all(g, g.run(imgs))[0], fresh[i][0], f"input {i} on the travelled context")
    g.close()
