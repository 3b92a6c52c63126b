"""The keypoint-batch cases (tests/keybatch_cases.py) are what they claim to be: checked with the binary32 restatement of
the level rule, and the CPU oracle takes every list.  No GPU."""
import numpy as np
import pytest

import keybatch_cases as kc
from hessgpu_amd import _abi
from oracle_lib import OracleSession


def test_table_is_the_oracles():
    o = OracleSession()
    assert (o.params.sigma0, o.params.dog_level_num) == (np.float32(1.6), 3)
    assert o.run(kc.images(1)) and len(o.geometry()) == kc.octaves() == 3
    lo, hi, osig = kc.level_table()
    half = kc.powf(2.0, np.float32(0.5) / np.float32(3))
    for li in range(9):
        ls = np.float32(np.float32(o.level_sigma(li % 3 + 1)) * osig[li])
        assert lo[li] == np.float32(ls / half) and hi[li] == np.float32(ls * half)
    assert np.all(lo[1:] > lo[:-1]) and np.all(hi[1:] > hi[:-1])


def test_case_a_covers_every_level_and_both_catch_alls():
    lo, hi, _ = kc.level_table()
    for case, flag in ((kc.case_a(), _abi.KEYS_ORIENTED), (kc.case_d(), _abi.KEYS_RECTANGLES)):
        assert tuple(len(k) for k in case) == kc.COUNTS_A
        allk = np.concatenate(case)
        m = kc.membership(allk, flag)
        assert m.shape == (9, sum(kc.COUNTS_A)) and m.any(axis=1).all(), "a level index without a key"
        s = kc.binned_scale(allk, flag)
        assert (s < lo[0]).any() and (s > hi[-1]).any(), "a catch-all without a key"
        assert ((s >= lo[0]) & (s < hi[0])).any() and ((s >= lo[-1]) & (s < hi[-1])).any()
        # the largest image alone reaches every level as well, so one image's list has every (level, seam) form
        assert kc.membership(case[3], flag).any(axis=1).all()
        assert m.sum(axis=0).max() <= 2


def test_case_b_fills_one_level_beyond_two_wavefronts():
    (k,) = kc.case_b()
    m = kc.membership(k, _abi.KEYS_ORIENTED)
    assert len(k) == 200 and m[1].sum() == 200 > 128 and m.sum() == 200
    assert (k[4::5].tobytes() == k[3::5].tobytes()) and len(np.unique(k["x"])) == 160
    assert np.array_equal(kc.list_order(k, _abi.KEYS_ORIENTED), np.arange(200))


def test_case_c_has_keys_listed_twice_and_nowhere():
    c0, c1 = kc.case_c()
    assert len(c0) == 45 and len(c1) == 46
    hits = [kc.membership(k, _abi.KEYS_ORIENTED).sum(axis=0) for k in (c0, c1)]
    assert set(np.unique(np.concatenate(hits))) <= {0, 1, 2}
    assert hits[1][7] == 0 and np.isnan(c1["s"][7]), "the NaN scale is listed nowhere"
    # (whether a seam's neighbours fall into both levels or into neither is the rounding's choice: both forms are legal,
    # and the list model states which one each key takes)
    for k, h in zip((c0, c1), hits):
        order = kc.list_order(k, _abi.KEYS_ORIENTED)
        assert len(order) == h.sum() and np.array_equal(np.bincount(order, minlength=len(k)), h)


@pytest.mark.parametrize("name", sorted(kc.CASES))
def test_oracle_takes_every_list(name):
    o = OracleSession(threads=4)
    for b, keys in enumerate(kc.CASES[name]()):
        if not len(keys):
            continue
        assert o.run(kc.image(b)[None])
        for flag in (0, 1):
            assert o.run_keypoints(keys, flag) == len(keys)
            assert len(o.fetch(0)[0]) == len(keys)
