"""bench.py --dump-outputs: what the last timed step delivered, written as .npy files within the size limit (the
writer alone, on made-up feature lists; tests/test_bench_contract_gpu.py runs it through bench.py on the GPU)."""
import importlib.util
import os

import numpy as np

from hessgpu_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_for_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _part(rng, counts, dim=128):
    n = sum(counts)
    keys = np.zeros(n, dtype=_abi.KEYPOINT_DTYPE)
    for f in ("x", "y", "s", "o", "response"):
        keys[f] = rng.random(n, dtype=np.float32)
    keys["level"] = rng.integers(0, 21, n)
    keys["type"] = rng.integers(0, 2, n)
    return counts, keys, rng.random((n, dim), dtype=np.float32)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_every_feature_of_every_rank_in_order(tmp_path):
    rng = np.random.default_rng(1)
    parts = [_part(rng, [300, 0, 200]), _part(rng, [400, 100, 50])]
    _bench().dump_outputs(str(tmp_path), parts)
    out = _load(tmp_path)
    assert sorted(out) == ["counts", "descriptors", "keypoints"]
    assert out["counts"].dtype == np.float64 and out["counts"].tolist() == [300, 0, 200, 400, 100, 50]
    keys = np.concatenate([p[1] for p in parts])
    assert out["keypoints"].dtype == np.float32 and out["keypoints"].shape == (1050, 7)
    for i, f in enumerate(_abi.KEYPOINT_DTYPE.names):
        assert np.array_equal(out["keypoints"][:, i], keys[f].astype(np.float32)), f
    assert out["descriptors"].dtype == np.float32
    assert np.array_equal(out["descriptors"], np.concatenate([p[2] for p in parts]))


def test_dump_above_the_limit_is_the_same_seeded_sample_every_time(tmp_path):
    rng = np.random.default_rng(2)
    parts = [_part(rng, [3000, 2000]), _part(rng, [4000, 1000])]
    bench = _bench()
    limit = 1 << 20
    outs = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), parts, limit=limit)
        assert sum(os.path.getsize(tmp_path / name / f) for f in os.listdir(tmp_path / name)) <= limit
        outs.append(_load(tmp_path / name))
    a, b = outs
    assert sorted(a) == ["counts", "descriptors", "keypoints", "sample_rows"]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    rows = a["sample_rows"].astype(np.int64)
    assert 1000 < len(rows) < 10000 and np.all(np.diff(rows) > 0) and rows[-1] < 10000
    assert a["counts"].tolist() == [3000, 2000, 4000, 1000]
    assert np.array_equal(a["descriptors"], np.concatenate([p[2] for p in parts])[rows])
    assert np.array_equal(a["keypoints"][:, 0], np.concatenate([p[1] for p in parts])["x"][rows])
