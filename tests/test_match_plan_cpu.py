"""The matcher's plan (hessgpu_amd/csrc/hess_match_plan.cpp: segments, chunks, scratch offsets, the plan buffer's tables) on the
CPU, under AddressSanitizer and UndefinedBehaviorSanitizer: tests/match_plan_main.cpp plans every case below, checks in each what
the kernels rely on (every (row block, segment) once in the multiply table, no empty segment, at most 60 tiles per segment, the
packing of rb | sg << 16, offsets as running sums, chunks that partition the list within MP_PAIRS and MP_SCRATCH) and prints the
plan.  Here the printed plans are compared with the restatement in tests/matcher_cases.py, by which the GPU tests place their tie
groups: the product is the authority, the restatement has to follow it."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import matcher_cases as mc
from test_stager_cpu import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hessgpu_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
MP_SCRATCH = 256 << 20
INT32_MAX = 2 ** 31 - 1
MAX_MATCH = 4096


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """The program, built once: plan(cases) runs it on lists of tokens -> one record per case, in order."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("neither g++ nor /opt/rocm/llvm/bin/clang++ is present")
    exe = str(tmp_path_factory.mktemp("match_plan") / "match_plan_main")
    build = subprocess.run([cxx] + FLAGS + ["-I", CSRC, os.path.join(CSRC, "hess_match_plan.cpp"),
                            os.path.join(ROOT, "tests", "match_plan_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return functools.partial(_run, exe)


def _run(exe, cases):
    text = "\n".join(" ".join(str(t) for t in c) for c in cases) + "\n"
    setarch = shutil.which("setarch")  # no address randomisation for this one program, as in test_stager_cpu
    r = subprocess.run(([setarch, os.uname().machine, "-R"] if setarch else []) + [exe], input=text, capture_output=True, text=True,
                       timeout=120)  # (the program carries the sanitizers' runtimes itself)
    assert r.returncode == 0 and f"PLAN OK {len(cases)}" in r.stdout, r.stdout[-2000:] + r.stderr[-6000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]] if w[0] != "PLAN" else []
        if w[0] == "single":
            out.append(dict(kind="single", n=(v[0], v[1]), plan=tuple(v[2:])))
        elif w[0] == "plan":
            keys = ("status", "jpp", "mm", "rs", "cp", "rm", "cm", "plan_bytes", "outn", "nchunks")
            out.append(dict(kind="list", chunks=[], jobs=[], **dict(zip(keys, v))))
        elif w[0] == "chunk":
            out[-1]["chunks"].append(dict(zip(("q0", "q1", "sps", "rs", "cp", "rm", "cm", "nwg", "nfin"), v)))
        elif w[0] == "job":
            out[-1]["jobs"].append(dict(zip(("idx", "n1", "n2", "nrb", "nsuper", "nseg", "sps", "rs", "cp", "rm", "cm"), v)))
    assert len(out) == len(cases)
    return out


def _list_case(sizes, pairs, mutual, typed=False, max_match=MAX_MATCH):
    """sizes: rows per set, or for typed sets four rows per set."""
    flat = [int(x) for s in sizes for x in (s if typed else (s,))]
    return ["list", int(typed), len(sizes), len(pairs), max_match, int(mutual)] + flat + [int(x) for p in pairs for x in p]


def _restated(pair_jobs, bounds, mutual):
    """The plan of a list by the restatement of matcher_cases: pair_jobs[p] = [(n1, n2) of each job of pair p], bounds = the
    (first pair, end pair) of every chunk -> (chunk records, job records) as the program prints them."""
    chunks, jobs = [], []
    for q0, q1 in bounds:
        sizes = [(a, b) if a and b else (0, 0) for p in range(q0, q1) for a, b in pair_jobs[p]]
        cap = mc.chunk_sps(sizes)
        c = dict(q0=q0, q1=q1, sps=cap, rs=0, cp=0, rm=0, cm=0, nwg=0, nfin=0)
        for n1, n2 in sizes:
            j = dict(idx=len(jobs), n1=n1, n2=n2, nrb=0, nsuper=0, nseg=0, sps=0, rs=0, cp=0, rm=0, cm=0)
            if n1:
                nrb, nsuper = -(-n1 // mc.ROWS), -(-n2 // mc.SUPER)
                nseg, psps = mc.pair_seg(nsuper, cap)
                j.update(nrb=nrb, nsuper=nsuper, nseg=nseg, sps=psps, rs=c["rs"], cp=c["cp"], rm=c["rm"], cm=c["cm"])
                c["rs"] += n1 * nseg
                c["cp"] += nrb * n2 if mutual else 0
                c["rm"] += n1
                c["cm"] += n2 if mutual else 0
                c["nwg"] += nrb * nseg
                c["nfin"] += -(-n1 // 256) + (-(-n2 // 32) if mutual else 0)
            jobs.append(j)
        chunks.append(c)
    return chunks, jobs


def _scratch(c):
    return 12 * (c["rs"] + c["cp"]) + 4 * (c["rm"] + c["cm"])


def _check_list(got, pair_jobs, bounds, mutual, set1_rows, max_match=MAX_MATCH):
    jpp = len(pair_jobs[0])
    chunks, jobs = _restated(pair_jobs, bounds, mutual)
    assert got["status"] == 0 and got["jpp"] == jpp and got["nchunks"] == len(bounds)
    assert got["chunks"] == chunks, [(a, b) for a, b in zip(got["chunks"], chunks) if a != b][:2]
    assert got["jobs"] == jobs, [(a, b) for a, b in zip(got["jobs"], jobs) if a != b][:2]
    mm = max(min(n, max_match) for n in set1_rows)
    assert got["mm"] == mm
    for k in ("rs", "cp", "rm", "cm"):
        assert got[k] == max([1] + [c[k] for c in chunks])
    assert got["plan_bytes"] == max(64 * jpp * (c["q1"] - c["q0"]) + 8 * (c["nwg"] + c["nfin"] + (c["q1"] - c["q0"] if jpp == 4 else 0))
                                    for c in chunks)
    assert got["outn"] == max(mc.BANK_CHUNK + (c["q1"] - c["q0"]) * mm * 2 for c in chunks)
    return chunks, jobs


def _every_64th(npairs):
    return [(k, min(k + mc.BANK_CHUNK, npairs)) for k in range(0, npairs, mc.BANK_CHUNK)]


def test_single_pairs_against_single_plan(plan):
    rng = np.random.RandomState(19)
    sizes = list(mc.MATRIX_CORE_SIZES) + list(mc.STRADDLE) + [tuple(int(x) for x in rng.randint(1, 40001, size=2)) for _ in range(4000)]
    got = plan([["single", n1, n2, k & 1] for k, (n1, n2) in enumerate(sizes)])
    differ = [(g["n"], g["plan"], mc.single_plan(*g["n"])) for g in got if g["plan"] != mc.single_plan(*g["n"])]
    assert not differ, (len(differ), differ[:5])
    assert [g["n"] for g in got] == sizes
    assert max(g["plan"][3] for g in got) == mc.MAX_SPS and max(g["plan"][2] for g in got) > 100      # the sweep reaches the cap


def test_bank_lists_against_the_restatement(plan):
    sizes = [len(s) for s in mc.bank_sets()]
    assert sizes == list(mc.BANK_SIZES) + [300]
    allp, big = [tuple(p) for p in mc.bank_all_pairs()], [tuple(p) for p in mc.bank_big_chunk_pairs()]
    got = plan([_list_case(sizes, pairs, mutual) for pairs in (allp, big) for mutual in (1, 0)])
    for k, (pairs, mutual) in enumerate((p, m) for p in (allp, big) for m in (1, 0)):
        jobs_of = [[(sizes[a], sizes[b])] for a, b in pairs]
        # the chunks end at every 64th pair, each at the cap chunk_sps gives its slice, every job with pair_seg's segments
        chunks, jobs = _check_list(got[k], jobs_of, _every_64th(len(pairs)), mutual, [sizes[a] if sizes[b] else 0 for a, b in pairs])
        assert all(_scratch(c) <= MP_SCRATCH for c in chunks)
        if pairs is allp:
            assert len(chunks) == 2 and {c["sps"] for c in chunks} <= {1, 2, 6}          # (test_geometry_of_the_cases)
        else:
            # one chunk at the cap of 15, with jobs of 2 x 13 (3100 columns) and 2 x 15 (3825 columns)
            assert len(chunks) == 1 and chunks[0]["sps"] == mc.MAX_SPS
            segs = {j["n2"]: (j["nseg"], j["sps"]) for j in got[k]["jobs"]}
            assert segs == {1500: (1, 12), 3100: (2, 13), 3825: (2, 15)}


def test_typed_bank_lists_against_the_restatement(plan):
    import matcher_type_cases as tc

    allp, big = [tuple(p) for p in mc.bank_all_pairs()], [tuple(p) for p in mc.bank_big_chunk_pairs()]
    cases, what = [], []
    for kind in ("random", "position"):
        groups = [np.bincount(tc.classes(t), minlength=4).tolist() for t in tc.bank_types(kind)]
        assert [sum(g) for g in groups] == list(mc.BANK_SIZES) + [300]
        for pairs in (allp, big):
            for mutual in (1, 0):
                cases.append(_list_case(groups, pairs, mutual, typed=True))
                what.append((kind, groups, pairs, mutual))
    got = plan(cases)
    for g, (kind, groups, pairs, mutual) in zip(got, what):
        jobs_of = [[(groups[a][c], groups[b][c]) for c in range(4)] for a, b in pairs]      # four jobs per pair, one per class
        rows = [sum(groups[a]) if sum(groups[b]) else 0 for a, b in pairs]
        chunks, jobs = _check_list(g, jobs_of, _every_64th(len(pairs)), mutual, rows)
        for j, (n1, n2) in zip(g["jobs"], (s for p in jobs_of for s in p)):
            assert (j["n1"], j["n2"]) == ((n1, n2) if n1 and n2 else (0, 0))                 # a class absent on either side: no work
        if pairs is big:
            # one chunk of more than 64 jobs (test_bank_chunk_of_more_than_64_jobs_at_the_segment_cap).  It lands at the cap
            # with the types by position: 164 jobs, 7 456 (row block, super tile) units / 512 workgroups -> 15.  The random
            # types split the work over four classes (sum of p^2 = 0.305 of the untyped 16 018): 256 jobs, 5 625 units -> 11
            jobs_with_work = sum(1 for j in g["jobs"] if j["n1"])
            assert len(chunks) == 1 and jobs_with_work > mc.BANK_CHUNK
            assert (chunks[0]["sps"], jobs_with_work, chunks[0]["nwg"] > 0) == {"position": (mc.MAX_SPS, 164, True),
                                                                                 "random": (11, 256, True)}[kind]
    absent = [j for g in got for j in g["jobs"] if not j["n1"]]
    assert absent                                                                               # ("position": class 0 / class 3 absent)


def test_sizes_without_memory_behind_them(plan):
    """Figures by arithmetic.  60 000 x 60 000 with mutual best: 235 row blocks x 60 000 columns = 14.1 M column partials of 12
    bytes, 169 MB, so a second pair would pass MP_SCRATCH (256 MiB): every pair is a chunk of its own.  100 000 x 100 000: 391 x
    100 000 = 39.1 M column partials, 469 MB -- above the budget, a chunk of its own, accepted (44.4 M entries < 2^31).
    800 000 x 800 000: 3 125 x 800 000 = 2.5 * 10^9 column partials > INT32_MAX: too big."""
    got = plan([_list_case([60000], [(0, 0)] * 7, 1), _list_case([100000], [(0, 0)], 1), _list_case([800000], [(0, 0)], 1),
                 _list_case([60000], [(0, 0)] * 14, 0)])
    chunks, jobs = _check_list(got[0], [[(60000, 60000)]] * 7, [(k, k + 1) for k in range(7)], 1, [60000] * 7)
    assert all(c["cp"] == 235 * 60000 and 12 * c["cp"] > 169e6 and MP_SCRATCH / 2 < _scratch(c) <= MP_SCRATCH for c in chunks)
    chunks, jobs = _check_list(got[1], [[(100000, 100000)]], [(0, 1)], 1, [100000])
    assert chunks[0]["cp"] == 391 * 100000 and _scratch(chunks[0]) > MP_SCRATCH and chunks[0]["rs"] + chunks[0]["cp"] <= INT32_MAX
    assert (jobs[0]["nrb"], jobs[0]["nsuper"], jobs[0]["nseg"], jobs[0]["sps"]) == (391, 782, 53, 15)
    assert got[2]["status"] == -1 and 3125 * 800000 > INT32_MAX
    # without mutual best there are no column partials: the row states of a pair are 60 000 x 32 segments x 12 bytes = 23 MB, and
    # the chunk ends before the pair that would pass the budget
    per_pair = 12 * 60000 * 32 + 4 * 60000
    fit = MP_SCRATCH // per_pair
    assert 1 < fit < 14
    bounds = [(k, min(k + fit, 14)) for k in range(0, 14, fit)]
    _check_list(got[3], [[(60000, 60000)]] * 14, bounds, 0, [60000] * 14)
