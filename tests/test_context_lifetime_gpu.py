"""The life of an extraction context: created, made to allocate every buffer hess_ctx has, destroyed -- many times in one
process.  Every cycle must give the first cycle's bytes, device memory must not grow from cycle to cycle, node-shared result
buffers must leave nothing behind, and a refused hess_create must leave the process as it was.  (Destroying a context
while a batch is pending is not tried: include/hess_abi.h does not say whether that is allowed.)"""
import contextlib
import ctypes as C
import os
import uuid

import numpy as np
import pytest

import fixtures

pytestmark = pytest.mark.gpu

W, H, B = 320, 240, 3
SHM = "/dev/shm"


@contextlib.contextmanager
def _env(**values):
    """The developer switches are read when the context is created: set for that moment, then put back."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def images():
    return np.stack([fixtures.synthetic_blobs(W, H, i) for i in range(B)])


@pytest.fixture(scope="module")
def pinned(images):
    import torch
    return torch.from_numpy(images).pin_memory()


def _used():
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free


def _results(ctx, n):
    return [(ctx.count(i),) + tuple(a.tobytes() for a in ctx.fetch(i)) for i in range(n)]


def _dev_ctx(**overrides):
    import hessgpu_amd
    return hessgpu_amd.HessContext(0, dev_switches=True, **overrides)


def _cycle(images, pinned):
    """-> (the results of every run, device bytes the first context held just before its close())."""
    out = []
    with _env(HESS_INITIAL_CAP="64"):
        c = _dev_ctx()
    c.reserve(W, H, B)
    c.run(images)
    assert c.regrown() > 0, "HESS_INITIAL_CAP did not make the feature storage grow"
    out.append(_results(c, B))
    c.submit_host(images)                                   # pageable pixels: the stager and the pinned staging buffer
    c.wait()
    out.append(_results(c, B))
    lists = [c.fetch(i)[0][:40] for i in range(B)]
    c.set_keypoints_batch(lists)                            # a keypoint list per image of the next batch
    c.run(images)
    out.append(_results(c, B))
    c.run_keypoints(lists[0][:20])                          # ... and a list on the current image
    out.append(_results(c, 1))
    c.set_descriptor_format("u8")
    c.run(images)
    out.append(_results(c, B))
    c.set_descriptor_format("f32")
    c.profile_enable(True)
    c.run(images)
    assert c.profile()["gauss"]["launches"] > 0
    out.append(_results(c, B))
    before = _used()
    c.close()
    footprint = before - _used()
    with _env(HESS_DELIVERY="dma"):
        c = _dev_ctx()
    c.submit_host(ptr=pinned.data_ptr(), batch=B, height=H, width=W)   # pinned pixels, uploaded beside the queues
    c.wait()
    out.append(_results(c, B))
    c.close()
    c = _dev_ctx(first_octave=-1)                           # the up-sampled plane
    c.run(images)
    out.append(_results(c, B))
    c.close()
    return out, footprint


@pytest.fixture(scope="module")
def first_cycle(images, pinned):
    return _cycle(images, pinned)[0]


def test_twelve_cycles_give_the_same_bytes_and_no_growth(images, pinned, first_cycle):
    assert all(n > 0 for run in first_cycle for n, *_ in run)
    plain = first_cycle[0]
    assert first_cycle[1] == plain and first_cycle[5] == plain and first_cycle[6] == plain   # one path, four ways in
    used, footprints = [], []
    for k in range(12):
        got, footprint = _cycle(images, pinned)
        assert got == first_cycle, f"cycle {k} differs from the first"
        used.append(_used())
        footprints.append(footprint)
    growth = used[-1] - used[1]
    print(f"footprint of one live context {footprints[-1]} bytes (all cycles: {sorted(set(footprints))}); "
          f"in use after close() 2: {used[1]}, after close() 12: {used[-1]}, growth {growth}")
    assert footprints[-1] > 0
    assert growth < footprints[-1] / 4, (growth, footprints[-1])


@pytest.mark.parametrize("as_files", [False, True], ids=["shm", "files"])
def test_shared_result_buffers_leave_nothing_behind(images, first_cycle, tmp_path, as_files):
    extra = dict(HESS_SHARE_FORCE_FILE="1", HESS_SHARE_DIR=str(tmp_path)) if as_files else {}
    with _env(**extra):
        for k in range(4):
            name = f"hess_lifetime_{uuid.uuid4().hex}"
            c = _dev_ctx()
            c.share_results(name)
            c.run(images)
            assert _results(c, B) == first_cycle[0]
            assert [f for f in os.listdir(SHM) if f.startswith(name)]
            assert bool(list(tmp_path.iterdir())) == as_files
            c.close()
            assert not [f for f in os.listdir(SHM) if f.startswith(name)] and not list(tmp_path.iterdir()), k


def test_fifty_refused_creates_then_a_context_that_works(images, first_cycle):
    import hessgpu_amd
    from hessgpu_amd.session import make_params
    lib, fns = hessgpu_amd.load_library(dev=True), hessgpu_amd.functions(dev=True)
    ndev = lib.hess_device_count()
    for k in range(50):
        p, device = make_params(fns["default_params"]), 0
        if k % 4 == 0:
            p.abi_version = 99
        elif k % 4 == 1:
            p.reserved[1 + k % 5] = 1          # a non-zero reserved word
        elif k % 4 == 2:
            p.dog_level_num = 11 if k % 8 == 2 else -1
        else:
            device = ndev                      # one past the last ordinal
        assert not fns["create"](device, C.byref(p)), k
    c = _dev_ctx()
    c.run(images)
    assert _results(c, B) == first_cycle[0]
    c.close()
