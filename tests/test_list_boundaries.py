"""The list stages at their count-set seams, on the CPU: the oracle against the plain list model of tests/list_cases.py.

The kernels that turn detections into lists have seams that a count sets, not a pixel -- 32 768 list rows (two bodies of the
row scan), 16 Ki spilled records (the placement grid and its trailing loop), 4 096 entries (a top-K chunk and the look-back
over chunk edges), 16 384 keypoints (a pass of the one-workgroup feature scan), the feature scan's rounded chunk length.  The
oracle has none of these seams; this file (a) holds it to the model on every case, so that the model and the oracle's bytes,
which tests/test_list_boundaries_gpu.py compares the HIP path with, are two independent statements of one answer, (b) asserts
from the untruncated list that every case reaches the seam it is there for, and (c) shows for each of the eight wrong
versions (list_cases.WRONG) a named case on which the oracle does not follow it.

One note on (c): "n == K treated as below K" alone is not observable -- with n == K either reading keeps every entry in list
order.  The switch `cut_strict` states the other half of that line, the cut sought with > where >= is meant, and a K that
equals the number of entries down to some key, with entries below it, tells the two apart.
"""
import hashlib
from contextlib import closing

import pytest

import list_cases as L
from oracle_lib import OracleSession

CASES = L.cases()
_FULL = {}     # untruncated oracle runs, shared by the cases of one input: (input, parameters) -> [Result per image]


def oracle_runner(case):
    imgs = case.image()
    digest = hashlib.md5(imgs.tobytes()).hexdigest()

    def run(kw):
        key = (digest, imgs.shape, tuple(sorted(kw.items())))
        if key in _FULL:
            return _FULL[key][case.index]
        with closing(OracleSession(threads=16, keep_levels=False, **kw)) as o:
            counts = o.run(imgs)
            res = [L.result_of(o, counts, b) for b in range(len(imgs))]
        if kw == case.base:
            _FULL[key] = res
        return res[case.index]

    return run


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_follows_the_list_model_and_the_case_reaches_its_seam(name):
    case = CASES[name]
    st = L.check_case(oracle_runner(case), case)
    L.check_reach(st, case)


# wrong version -> the case that catches it
CAUGHT = {
    "tie_high": "C: n 8192 cut in chunk 0",
    "tie_quota_per_chunk": "C: n 8192 cut in chunk 1",
    "ties_before_ignored": "C: n 12600 cut in chunk 2",
    "cut_strict": "C: n 8192 cut in whole run",
    "dropped_level_advances": "A: 43008 rows h1 levels",
    "level_without_base": "A: 33600 rows dog 6 h0 levels",
    "spill_dropped": "B: grid 1240x480 batch of three, image 0",
    "carry_lost": "D: one workgroup, h1 after the reshape",
}


def test_every_wrong_version_has_its_case():
    assert set(CAUGHT) == set(L.WRONG) and len(L.WRONG) == 8 and set(CAUGHT.values()) <= set(CASES)


@pytest.mark.parametrize("switch", list(CAUGHT))
def test_wrong_version_is_caught(switch):
    case = CASES[CAUGHT[switch]]
    with pytest.raises(L.Mismatch):
        L.check_case(oracle_runner(case), case, wrong={switch: True})


@pytest.mark.parametrize("switch", ["tie_high", "tie_quota_per_chunk", "ties_before_ignored"])
def test_tie_switches_are_silent_away_from_their_seam(switch):
    """Below K nothing is cut under any tie rule: what catches the tie switches is the cut inside a tie run at a chunk
    edge, not the length of the list."""
    case = CASES["C: n 4096 K n + 1"]
    L.check_case(oracle_runner(case), case, wrong={switch: True})
