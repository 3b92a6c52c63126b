"""A caller compiled against the REFERENCE's header works unchanged against this build's libsiftgpu.so.

tests/abi/abi_caller.cpp prints sizes, member offsets, enum values, and the results of calls made through the vtable /
constructor symbols the header it is compiled with declares (factory object as TestWin/SimpleSIFT.cpp:88-202, stack
object as HessGPU/hessgpucmd.cpp:27).  tests/golden/abi_caller_reference_header.txt is what it printed compiled with
-I <reference>/src/SiftGPU (SiftGPU.h:59-379 + config.h), linked to hessgpu_amd/libsiftgpu.so and run without a GPU;
regenerate it that way whenever abi_caller.cpp changes.  Here the caller is compiled with -I include/, linked to the
library and run: its output must be the stored one line by line, except that a machine with a GPU prints
"CreateContextGL full" for "none", and its stack object's RunSIFT runs and prints the library's verbose report (set
aside before the comparison: the run time differs from run to run).  With HESS_REFERENCE_DIR set to a checkout of the
reference, the caller is also compiled against the reference's own header and must print the same."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_caller_reference_header.txt")
LIBDIR = os.path.join(ROOT, "hessgpu_amd")


def _build_and_run(tmp_path, inc, name):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++11", "-O0", "-I", inc, os.path.join(ROOT, "tests", "abi", "abi_caller.cpp"), "-o", exe,
                    "-L", LIBDIR, "-lsiftgpu", "-lhessgpu", f"-Wl,-rpath,{LIBDIR}"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


def _is_run_report(line):
    """A line of the library's verbose report after a RunSIFT that ran (siftgpu_api.cpp: "#Features:", the run time, a
    blank line), not one of the caller's."""
    return re.fullmatch(r"#Features:\t\d+|RUN SIFT:\t\S+ms|", line) is not None


def test_caller_built_with_the_reference_header_runs_against_this_library(tmp_path):
    import torch

    import hessgpu_amd.build as hb

    hb.build_all()
    with open(GOLDEN) as f:
        ref = f.read().splitlines()
    if torch.cuda.is_available():   # (the stored output was made without a GPU: no context there, a loud 0)
        ref = ["CreateContextGL full" if l == "CreateContextGL none" else l for l in ref]
    own_all = _build_and_run(tmp_path, os.path.join(ROOT, "include"), "caller_own")
    own = [l for l in own_all if not _is_run_report(l)]
    assert any(l.startswith("#Features:") for l in own_all) == torch.cuda.is_available()   # with a device RunSIFT ran
    assert ref == own, "\n".join(f"{a!r} != {b!r}" for a, b in zip(ref, own) if a != b)
    ref_dir = os.environ.get("HESS_REFERENCE_DIR")
    if ref_dir:
        live = [l for l in _build_and_run(tmp_path, os.path.join(ref_dir, "src", "SiftGPU"), "caller_ref") if not _is_run_report(l)]
        assert live == own, "\n".join(f"{a!r} != {b!r}" for a, b in zip(live, own) if a != b)
    d = dict(l.rsplit(" ", 1) for l in ref if " " in l)
    assert d["sizeof SiftParam"] == "56" and d["sizeof SiftGPU"] == "168" and d["sizeof SiftKeypoint"] == "24"
    assert d["offsetof _timing"] == "120" and d["sizeof timing"] == "48" and d["SIFT_KEYPOINT_ITEMS"] == "6"
    assert "factory ok" in ref and "GetImageCount 3" in ref and "stack GetImageCount 1" in ref
    assert "after ParseParam: _dog_level_num 4 _dog_threshold 0.0100" in ref   # -d 4 -t 0.01 landed in the SiftParam members
    assert "RunSIFT(missing file) 0" in ref and "IsFullSupported consistent 1" in ref
    assert "stack RunSIFT(pixels) returned" in ref and ref[-1] == "done"
    assert ("CreateContextGL none" in own) == (not torch.cuda.is_available())   # no GPU: loud 0, not a fallback
