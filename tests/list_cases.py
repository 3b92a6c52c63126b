"""Inputs and a plain model for the LIST stages: the kernels that turn detections into lists (k_detect.hip: row_scan_block
with extrema_place_kernel, topk_select_kernel; k_feature.hip: feature_scan_kernel).  Each of them has a seam that is set by
a count, not by a pixel: 32 768 list rows per image (the register body of the row scan against the one that re-reads its
counts), 16 Ki spilled records (the placement grid against its trailing loop), 4 096 list entries (a top-K chunk, with the
look-back across chunk edges), 16 384 keypoints (a pass of the one-workgroup feature scan) and the feature scan's chunk
length, rounded to 1 024.  The inputs here are narrow strips of Gaussian dots that reach those counts; a plain helper module,
no tests in it.  tests/test_list_boundaries.py holds the CPU oracle to the model, tests/test_list_boundaries_gpu.py the HIP
path to the model and to the oracle's bytes.

The model (ListModel) is plain NumPy / Python written from DESIGN.md section 1 and the reference lines cited there
(SiftPyramid.cpp:201-278, PyramidCU.cpp:1283-1368, :780-796); it shares no code with oracle/hess_oracle.c or the kernels.  It
takes the UNTRUNCATED raw list of a session and its orientation count per keypoint and states the list order, the top-K
selection, the three level-truncation methods in both passes (np_restatement.DetectorModel states those rules and is
called) and the feature table.  Every stage is judged from the session's own previous stage: the list of a truncating
session against the model applied to the list of a second session with the same parameters and no truncation.

Each rule has a switch that states a wrong version (WRONG); the CPU test shows the case that catches each.  The wrong
versions are what a slip at the seam would compute, so some of them need the seam's number (the constants below).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np

import np_restatement as R
from hessgpu_amd import _abi

TOPK_CHUNK = 4096        # entries per top-K chunk
SCAN_PASS = 16384        # keypoints per pass of the one-workgroup feature scan
REGISTER_ROWS = 32768    # list rows per image up to which the row scan keeps its counts in registers
TASK_SLOTS = 64          # records a scan task owns before it spills
TASK_COLUMNS = 124       # columns of a scan strip
GRID_SPILL = 16384       # spilled records the placement launch covers without its trailing loop

WRONG = ("tie_high", "tie_quota_per_chunk", "ties_before_ignored", "cut_strict", "dropped_level_advances",
         "level_without_base", "spill_dropped", "carry_lost")


# ---- inputs --------------------------------------------------------------------------------------------------------------
def dot_field(w, h, period, sigma, amp=0.3, y0=0, y1=None, jitter_seed=None, skip=()):
    """Alternating bright / dark Gaussian dots on a grid of `period` pixels with centres in rows y0 + 3, y0 + 3 + period, ...
    below y1 (float64, zero background; the sum over the dots as two matrix products).  skip: indices of dots left out,
    counted row-major over the band's dot grid.  jitter_seed: amplitudes 0.3 .. 0.35 as test_gpu_parity._dot_grid has them."""
    y1 = h if y1 is None else y1
    cys, cxs = np.arange(y0 + 3, y1, period), np.arange(3, w, period)
    sign = np.where(((cxs[None, :] // period + (cys[:, None] - y0) // period) & 1) == 1, 1.0, -1.0)
    a = np.full(sign.shape, float(amp))
    if jitter_seed is not None:
        a += 0.05 * np.random.RandomState(jitter_seed).rand(*sign.shape)
    a *= sign
    if len(skip):
        a.reshape(-1)[np.asarray(skip, dtype=np.int64)] = 0.0
    gy = np.exp(-((np.arange(h)[:, None] - cys[None, :]) ** 2) / (2.0 * sigma * sigma))
    gx = np.exp(-((cxs[:, None] - np.arange(w)[None, :]) ** 2) / (2.0 * sigma * sigma))
    return gy @ a @ gx


def to_u8(field):
    """Grey 128 plus the field: bright and dark dots of one amplitude are mirror images of each other about 128, det-H is even
    in the sign of the plane, so both kinds get ONE top-K key -- the long tie runs come from that."""
    return np.clip(np.rint(128.0 + 255.0 * field), 0, 255).astype(np.uint8)


def strip(w, bands, skip=()):
    """Bands of dots one below the other: (rows, period, sigma, amplitude) each.  skip: (band, dot index) pairs."""
    h = sum(b[0] for b in bands)
    f, y0 = np.zeros((h, w)), 0
    for i, (rows, period, sigma, amp) in enumerate(bands):
        f += dot_field(w, h, period, sigma, amp, y0, y0 + rows, skip=[d for b, d in skip if b == i])
        y0 += rows
    return to_u8(f)


MIXED = ((8, 1.7), (12, 2.6), (16, 3.6), (32, 7.0))   # (period, sigma) of the mixed strip's bands of 256 rows


@lru_cache(maxsize=None)
def mixed_strip(h, w=64):
    """Dot sizes that spread the detections over the levels of two or three octaves (the -tc rules need several levels)."""
    return strip(w, [(min(256, h - y), *MIXED[(y // 256) % 4], 0.3) for y in range(0, h, 256)])


@lru_cache(maxsize=None)
def dense_grid(w, h, seed, flip=False):
    img = to_u8(dot_field(w, h, 6, 1.7, jitter_seed=seed))
    return img[::-1].copy() if flip else img


def in_batch_of_three(img, shift):
    """img as image 1 between a constant image and itself moved down by `shift` rows."""
    return np.stack([np.full_like(img, 128), img, np.roll(img, shift, axis=0)])


# ---- what a list says ------------------------------------------------------------------------------------------------------
def topk_key(raw):
    return ((raw["packed"] >> 16) & 0x7fff).astype(np.int64)


def strictly_ordered(raw):
    """List order: strictly increasing (level_index, row, col), hence no duplicates."""
    if len(raw) < 2:
        return True
    a = np.stack([raw["level_index"], raw["row"], raw["col"]], axis=1).astype(np.int64)
    d = a[1:] - a[:-1]
    lead = np.where(d[:, 0] != 0, d[:, 0], np.where(d[:, 1] != 0, d[:, 1], d[:, 2]))
    return bool((lead > 0).all())


def list_rows(geometry, dog):
    """NR: rows of the (level, row) list order of one image."""
    return dog * sum(h for _, h in geometry)


def task_spill(raw, geometry, dog, seg_rows, octaves=None):
    """-> (records beyond the TASK_SLOTS slots of their scan task, summed over the tasks; mask of those records in list order).
    A task is a strip of TASK_COLUMNS columns x a segment of seg_rows rows of one octave, all its detection levels."""
    spilled = np.zeros(len(raw), dtype=bool)
    for oc in range(len(geometry)) if octaves is None else octaves:
        idx = np.flatnonzero(raw["level_index"] // dog == oc)
        task = (raw["col"][idx] // TASK_COLUMNS).astype(np.int64) * (1 << 20) + raw["row"][idx] // seg_rows
        order = np.argsort(task, kind="stable")
        ts = task[order]
        start = np.flatnonzero(np.concatenate([[True], ts[1:] != ts[:-1]])) if len(ts) else np.zeros(0, dtype=np.int64)
        rank = np.arange(len(ts)) - np.repeat(start, np.diff(np.concatenate([start, [len(ts)]])))
        spilled[idx[order[rank >= TASK_SLOTS]]] = True
    return int(spilled.sum()), spilled


def take(raw, idx):
    """Entries idx of a list; -1 is a record nothing was written to (all zero)."""
    idx = np.asarray(idx, dtype=np.int64)
    out = np.zeros(len(idx), dtype=raw.dtype)
    out[idx >= 0] = raw[idx[idx >= 0]]
    return out


def orientation_counts(raw, keys, params):
    """Features per entry of `raw`, read off the keypoints the same session fetched: the features of one keypoint are
    consecutive and share level, position, scale, type and response; keypoints come in list order and one without an
    orientation is absent.  -> (counts, first feature of every entry).  Raises AssertionError when the keypoints are no
    such sequence -- that IS the feature table's order (PyramidCU.cpp:780-796)."""
    n = len(raw)
    counts, first = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    dog = int(params.dog_level_num) or 3
    sc = 2.0 ** (raw["level_index"] // dog + int(params.first_octave))
    off = 0.0 if params.lowe_origin else 0.5
    ex = sc * (raw["col"] + raw["dx"].astype(np.float64)) + off
    ey = sc * (raw["row"] + raw["dy"].astype(np.float64)) + off
    resp = (raw["packed"] >> 16).astype(np.uint16).view(np.float16).astype(np.float32)
    kx, ky, kl, kr = keys["x"].astype(np.float64), keys["y"].astype(np.float64), keys["level"], keys["response"]
    i = m = 0
    while m < len(keys):
        while i < n and not (kl[m] == raw["level_index"][i] and kr[m] == resp[i] and abs(kx[m] - ex[i]) <= sc[i] * 0.003 + 0.004
                             and abs(ky[m] - ey[i]) <= sc[i] * 0.003 + 0.004):
            first[i] = m
            i += 1
        assert i < n, f"feature {m} (level {kl[m]}, x {kx[m]}, y {ky[m]}) follows no list entry at or after its predecessor's"
        first[i] = m
        m0 = m
        while m < len(keys) and (kl[m], keys["x"][m], keys["y"][m], keys["s"][m]) == (kl[m0], keys["x"][m0], keys["y"][m0], keys["s"][m0]):
            m += 1
        counts[i] = m - m0
        i += 1
    first[i:] = len(keys)
    return counts, first


# ---- the model -------------------------------------------------------------------------------------------------------------
class ListModel:
    """params: anything with the fields of hess_params; geometry: the session's [(aligned width, height)]."""

    def __init__(self, params, geometry, seg_rows=24, **wrong):
        assert set(wrong) <= set(WRONG), wrong
        self.wrong = {k: bool(wrong.get(k)) for k in WRONG}
        self.m = R.DetectorModel(params)
        self.geometry = list(geometry)
        self.dog = self.m.dog
        self.nlev = self.dog * len(self.geometry)
        self.method, self.K = self.m.method, self.m.fct
        self.seg_rows = seg_rows
        self.topk = self.method == R.TRUNC_TOPK and self.K > 0
        self.rule = self.method != R.TRUNC_TOPK and self.K > 0

    # -- detection list ------------------------------------------------------------------------------------------------------
    def placed(self, raw):
        """Entries of the untruncated list that reach the list at all: every one of them.  spill_dropped: the WRONG version in
        which the records a scan task spills beyond the first GRID_SPILL of the image are never placed (their rows were
        counted, so the places stay empty)."""
        idx = np.arange(len(raw), dtype=np.int64)
        if self.wrong["spill_dropped"]:
            _, spilled = task_spill(raw, self.geometry, self.dog, self.seg_rows)
            late = np.flatnonzero(spilled)[GRID_SPILL:]
            idx[late] = -1
        return idx

    def level_counts(self, raw):
        return np.bincount(raw["level_index"], minlength=self.nlev).astype(np.int64)

    def select(self, raw):
        """-> indices into the untruncated list `raw` of the entries of the session's list, in its order."""
        idx = self.placed(raw)
        if self.topk:
            return idx[self._topk(topk_key(raw))]
        if self.rule:
            return self._first_pass(raw)
        return idx

    def _first_pass(self, raw):
        """GenerateFeatureList + the first LimitFeatureCount on the detection counts: a level stays whole or goes."""
        lvl = raw["level_index"].astype(np.int64)
        counts = self.level_counts(raw)
        if self.wrong["level_without_base"]:
            # the WRONG version: the level of list row i taken as i / h of its octave without the octave's first row -- right
            # in octave 0, past the octave's levels from octave 1 on (clamped to the last level here)
            oc = lvl // self.dog
            hs = np.array([h for _, h in self.geometry], dtype=np.int64)
            base = np.concatenate([[0], np.cumsum(self.dog * hs)])[:-1]
            row = base[oc] + (lvl % self.dog) * hs[oc] + raw["row"]
            seen = np.minimum(oc * self.dog + row // hs[oc], self.nlev - 1)
            c_seen = np.bincount(seen, minlength=self.nlev)
            after = np.array(self.m.reduce_first(c_seen.tolist()))
            row_kept = (after == c_seen)[seen]
            pos = np.cumsum(row_kept) - row_kept
            out = np.full(int(after.sum()), -1, dtype=np.int64)
            ok = row_kept & (after[lvl] != 0) & (pos < len(out))
            out[pos[ok]] = np.flatnonzero(ok)
            return out
        kept = np.array(self.m.reduce_first(counts.tolist())) > 0
        if self.wrong["dropped_level_advances"]:
            # the WRONG version: the rows of a dropped level still advance the offsets, so a kept entry keeps the place it
            # has in the untruncated list and the places of the dropped ones stay empty
            out = np.full(int(counts[kept].sum()), -1, dtype=np.int64)
            ok = kept[lvl] & (np.arange(len(raw)) < len(out))
            out[np.flatnonzero(ok)] = np.flatnonzero(ok)
            return out
        return np.flatnonzero(kept[lvl])

    def cut(self, key):
        """-> (cut key, sure keeps, ties, need): the K largest keys are those above the cut and `need` of the ties at it."""
        order = np.sort(key)[::-1]
        cut = int(order[self.K - 1])
        sure, ties = int((key > cut).sum()), int((key == cut).sum())
        return cut, sure, ties, self.K - sure

    def _topk(self, key):
        """SelectTopK, PyramidCU.cpp:1881-1987: skipped below K entries; otherwise the K largest keys, list order kept.
        PROJECT: equal keys go to the lower list index."""
        n, K, w = len(key), self.K, self.wrong
        if n < K:
            return np.arange(n)
        cut, sure, ties, need = self.cut(key)
        if w["cut_strict"]:
            # the WRONG version: the cut bin sought with "entries down to this key > K" where >= is meant.  Where the keys
            # down to some value are exactly K, no bin qualifies and nothing is cut.
            if sure + ties == K:
                return np.arange(n)
        is_sure, is_tie = key > cut, key == cut
        rank = np.cumsum(is_tie) - is_tie                       # ties before the entry
        if w["tie_high"]:
            return np.flatnonzero(is_sure | (is_tie & (rank >= ties - need)))
        chunk = np.arange(n) // TOPK_CHUNK
        first_of_chunk = np.searchsorted(chunk, np.arange(chunk.max() + 1))
        local = rank - rank[first_of_chunk][chunk]              # ties before the entry inside its chunk
        if w["tie_quota_per_chunk"]:                            # WRONG: every chunk keeps min(its ties, need)
            return np.flatnonzero(is_sure | (is_tie & (local < need)))
        if w["ties_before_ignored"]:
            # WRONG: the look-back's tie sum taken as 0 -- every chunk keeps its first `need` ties and counts its places from
            # the sure keeps before it alone; the kept total is that of the last chunk
            esure = np.cumsum(is_sure) - is_sure
            keep = is_sure | (is_tie & (local < need))
            pos = esure + np.minimum(local, need)
            last = chunk == chunk.max()
            total = int(is_sure.sum()) + min(int((is_tie & last).sum()), need)
            out = np.full(total, -1, dtype=np.int64)
            ok = keep & (pos < total)
            out[pos[ok]] = np.flatnonzero(ok)                   # (ascending: a later chunk overwrites an earlier one)
            return out
        return np.flatnonzero(is_sure | (is_tie & (rank < need)))

    def topk_reach(self, key):
        """Where the cut falls: the last kept tie, its chunk, the ties before that chunk and `need`."""
        cut, sure, ties, need = self.cut(key)
        tie_at = np.flatnonzero(key == cut)
        last = int(tie_at[need - 1])
        ck = last // TOPK_CHUNK
        before = int((tie_at < ck * TOPK_CHUNK).sum())
        in_chunk = [int(((tie_at // TOPK_CHUNK) == c).sum()) for c in range((len(key) - 1) // TOPK_CHUNK + 1)]
        sure_in = [int(((np.flatnonzero(key > cut) // TOPK_CHUNK) == c).sum()) for c in range(len(in_chunk))]
        return dict(cut=cut, sure=sure, ties=ties, need=need, last_kept_tie=last, chunk=ck, ties_before_chunk=before,
                    ties_in_chunk=in_chunk, sure_in_chunk=sure_in)

    # -- feature table -------------------------------------------------------------------------------------------------------
    def features(self, levels, counts):
        """levels, counts: level index and orientation count of every entry of the session's list.  -> [(entry, rank)] of the
        features it delivers: feature m belongs to entry i with rank q where m = sum of the counts before i, + q
        (PyramidCU.cpp:780-796); under a -tc rule LimitFeatureCount runs again on the expanded counts (SiftPyramid.cpp:140-147)."""
        levels, counts = np.asarray(levels, dtype=np.int64), np.asarray(counts, dtype=np.int64)
        if self.wrong["carry_lost"]:
            # the WRONG version: the running feature count starts again at every pass of SCAN_PASS keypoints, and the total is
            # the last pass's
            table, total = {}, 0
            for p0 in range(0, len(counts), SCAN_PASS):
                c = counts[p0:p0 + SCAN_PASS]
                off = np.cumsum(c) - c
                for i in np.flatnonzero(c):
                    for q in range(c[i]):
                        table[int(off[i]) + q] = (p0 + int(i), q)
                total = int(c.sum())
            return [table[m] for m in range(total)]
        multi = np.bincount(levels, weights=counts, minlength=self.nlev).astype(np.int64)
        kept = np.array(self.m.reduce_second(multi.tolist()) if self.rule else multi) > 0
        return [(int(i), q) for i in np.flatnonzero(kept[levels] & (counts > 0)) for q in range(counts[i])]


def pick_threshold(method, counts, dog, intent):
    """A feature_count_threshold for a -tc method from the untruncated level counts: 'nothing' drops no level, 'levels' drops
    at least two non-empty levels, one of them in octave 1, and keeps at least two, 'single' leaves one non-empty level.
    Candidates are the partial sums of the counts and their neighbours; the first that does it is taken (the test then
    asserts the intent on the session's own list)."""
    counts = [int(c) for c in counts]
    filled = [i for i, c in enumerate(counts) if c]
    sums = {sum(counts[:i]) for i in range(len(counts) + 1)} | {sum(counts[i:]) for i in range(len(counts) + 1)}
    for t in sorted({s + d for s in sums for d in (-1, 0, 1)} | {1}):
        if t <= 0:
            continue
        kept = R.DetectorModel(dict(truncate_method=method, feature_count_threshold=t, max_orientation=1)).reduce_first(counts)
        left = [i for i in filled if kept[i]]
        gone = [i for i in filled if not kept[i]]
        if intent_holds(intent, left, gone, dog):
            return t
    raise AssertionError(f"no threshold for {intent} with method {method} on {counts}")


def intent_holds(intent, left, gone, dog):
    if intent == "nothing":
        return not gone
    if intent == "single":
        return len(left) == 1
    return len(gone) >= 2 and any(dog <= i < 2 * dog for i in gone) and len(left) >= 2


def scan_chunks(n, capacity):
    """The multi-chunk form of the feature scan: -> (chunks launched, chunk length, chunks that hold keypoints)."""
    nchunk = min(16, max(1, capacity // 4096))
    clen = (((n + nchunk - 1) // nchunk) + 1023) & ~1023
    return nchunk, clen, (n + clen - 1) // clen if clen else 0


def planned_capacity(geometry, dog):
    """Raw-list records a fresh context plans per image (hess_plan.hip: a 32nd of the detection pixels, at least 16 Ki)."""
    return max(16384, dog * sum(w * h for w, h in geometry) // 32)


# ---- cases -----------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name seam image index base trunc seg_rows reach")


def _case(name, seam, image, base=None, trunc=None, index=0, seg_rows=12, **reach):
    """image: a function -> [B, H, W] u8; index: the image judged; base: parameters of both sessions; trunc: None, a dict
    of truncation parameters, or a function of (model, untruncated list) -> dict; seg_rows: rows of a scan segment when the
    batch is RUN (12 for one or two images, 24 from three on; a submitted batch always has 24)."""
    return Case(name, seam, image, index, base or {}, trunc, seg_rows, reach)


T = dict(zip(("h0", "h1", "low", "topk"), (_abi.TRUNC_HIGHEST_0, _abi.TRUNC_HIGHEST_1, _abi.TRUNC_LOWEST, _abi.TRUNC_TOPK)))

# One-size strips with a list of exactly n entries: 64 wide, a band of 256 rows of strong dots (amplitude 0.45: sure keeps)
# over `rows` rows of dots of amplitude 0.3 (period 8, sigma 1.7: one top-K key for six of the seven detections of a dot row),
# at tex_max_dim 16384.  Searched with the oracle: the height first (a dot row is 7 entries), then single dots of column 3
# taken out of the second band, which move n by one each.  n -> (rows, dots removed from band 1)
TIE_SKIP = (323, 347, 371, 395, 419, 443, 467, 491)
TIE_STRIPS = {4096: (4144, 7), 4097: (4144, 6), 8191: (8824, 7), 8192: (8824, 6), 12600: (13864, 8)}
TIE_BASE = dict(tex_max_dim=16384)
# The dense strip (period 6, sigma 1.7) with a list of 15 361 entries = 15 x 1024 + 1 in a plane that plans 15 scan chunks:
# 4620 rows of dots over grey rows up to 8190, three inner dots removed (9 entries each; searched with the oracle).
DENSE_15361 = (4620, ((0, 40 * 11 + 5), (0, 80 * 11 + 5), (0, 120 * 11 + 5)))
# The dense grid of test_gpu_parity._dot_grid without its noise, 1240 wide: the smallest height (in steps of a dot row) at
# which one image, scanned in 12-row segments, spills more than GRID_SPILL records from the tasks of octave 0 (1092: 16 361).
GRID_SINGLE_H = 1098
GRID_KW = dict(dog_threshold=0.0004, edge_threshold=60.0, compute_descriptors=0, max_orientation=1)


@lru_cache(maxsize=None)
def tie_strip(n, pad_to=None):
    rows, k = TIE_STRIPS[n]
    bands = [(256, 8, 1.7, 0.45), (rows, 8, 1.7, 0.3)]
    if pad_to:
        bands.append((pad_to - 256 - rows, 8, 1.7, 0.0))
    return strip(64, bands, [(1, d) for d in TIE_SKIP[:k]])


@lru_cache(maxsize=None)
def weak_strip():
    """A band of the weaker dots, more than two chunks of entries long, between two strong bands."""
    return strip(64, [(4000, 8, 1.7, 0.45), (6400, 8, 1.7, 0.3), (1000, 8, 1.7, 0.45)])


@lru_cache(maxsize=None)
def dense_strip():
    """More than SCAN_PASS keypoints in two levels: dense dots for level 0 and larger ones for level 1, so many that level 1's
    FEATURES outnumber the detections of both -- a -tc threshold between the two cuts only after the reshape."""
    return strip(64, [(3600, 6, 1.7, 0.3), (4592, 8, 2.6, 0.3)])


@lru_cache(maxsize=None)
def dense_15361():
    rows, skip = DENSE_15361
    return strip(64, [(rows, 6, 1.7, 0.3), (8190 - rows, 6, 1.7, 0.0)], skip)


def _tie_need(where):
    """K with the cut inside the run of the most frequent key, from the untruncated list."""
    def trunc(model, raw, counts):
        key = topk_key(raw)
        vals, cnt = np.unique(key, return_counts=True)
        tie = int(vals[np.argmax(cnt)])
        at = np.flatnonzero(key == tie)
        per = np.bincount(at // TOPK_CHUNK, minlength=4)
        need = {"chunk 0": per[0] // 2, "end of chunk 0": per[0], "first of chunk 1": per[0] + 1,
                "chunk 1": per[0] + per[1] // 2, "chunk 2": per[0] + per[1] + per[2] // 2, "whole run": len(at)}[where]
        return dict(truncate_method=T["topk"], feature_count_threshold=int((key > tie).sum() + need))
    return trunc


def _k_relative(d):
    return lambda model, raw, counts: dict(truncate_method=T["topk"], feature_count_threshold=len(raw) + d)


def _k_in_strong(model, raw, counts):
    """The cut inside a run of a strong band's keys, the last kept tie beyond the weak band: the most frequent key above every
    key of the weak band's chunk and below the largest one, all but 50 of its entries kept."""
    key = topk_key(raw)
    weak = int(key[TOPK_CHUNK:2 * TOPK_CHUNK].max())
    vals, cnt = np.unique(key[(key > weak) & (key < key.max())], return_counts=True)
    tie = int(vals[np.argmax(cnt)])
    return dict(truncate_method=T["topk"], feature_count_threshold=int((key > tie).sum() + cnt.max() - 50))


def _tc(method, intent):
    def trunc(model, raw, counts):
        return dict(truncate_method=T[method], feature_count_threshold=pick_threshold(T[method], model.level_counts(raw), model.dog, intent))
    return trunc


def _tc_second(method):
    """A threshold that leaves every level to the first pass that the second one, on the expanded counts, then drops: below
    the expanded total, above the detection total of the levels the first pass keeps."""
    def trunc(model, raw, counts):
        c = model.level_counts(raw)
        multi = np.bincount(raw["level_index"], weights=counts, minlength=model.nlev).astype(np.int64)
        for t in sorted({int(s) + d for s in list(np.cumsum(c)) + list(np.cumsum(c[::-1])) + list(np.cumsum(multi)) + list(np.cumsum(multi[::-1]))
                         for d in (-1, 0, 1)}):
            if t <= 0:
                continue
            m = R.DetectorModel(dict(truncate_method=T[method], feature_count_threshold=t, max_orientation=2))
            k1 = np.array(m.reduce_first(c.tolist())) > 0
            k2 = np.array(m.reduce_second((multi * k1).tolist())) > 0
            if c[k1].sum() > SCAN_PASS and (k1 & (multi > 0) & ~k2).any() and (k2 & (multi > 0)).any() and c[k1].sum() < t < (multi * k1).sum():
                return dict(truncate_method=T[method], feature_count_threshold=t)
        raise AssertionError(f"no threshold cuts after the reshape: {c}, {multi}")
    return trunc


def cases():
    """name -> Case.  Groups: A row scan, B placement, C top-K, D feature scan."""
    out = {}

    def add(name, seam, image, **kw):
        out[name] = _case(name, seam, image, **kw)

    # ---- A: both bodies of the row scan and the seam between them
    one = lambda f, *a: (lambda: f(*a)[None])
    add("A: 32768 rows", "rows", one(mixed_strip, 8192), base=dict(dog_level_num=4, octave_num=1, tex_max_dim=8192), rows=32768, levels=(2, 1))
    add("A: 32772 rows", "rows", one(mixed_strip, 8193), base=dict(dog_level_num=4, octave_num=1, tex_max_dim=8193), rows=32772, levels=(2, 1))
    for tag, h, base, rows in (("43008 rows", 8192, dict(tex_max_dim=8192), 43008), ("33600 rows dog 6", 3200, dict(dog_level_num=6), 33600)):
        for det in (0, 1):
            b = dict(base, detector=det)
            mode = "dog" if det else "hessian"
            add(f"A: {tag} {mode}", "rows", one(mixed_strip, h), base=b, rows=rows, levels=(4, 2))
            add(f"A: {tag} {mode} in a batch", "rows", (lambda h=h: in_batch_of_three(mixed_strip(h), 4)), base=b, index=1, seg_rows=24,
                rows=rows, levels=(4, 2))
        for method in ("h0", "h1", "low"):
            for intent in ("nothing", "levels", "single"):
                add(f"A: {tag} {method} {intent}", "rows", one(mixed_strip, h), base=base, trunc=_tc(method, intent), rows=rows,
                    levels=(4, 2), intent=intent)
        add(f"A: {tag} h1 levels in a batch", "rows", (lambda h=h: in_batch_of_three(mixed_strip(h), 4)), base=base, index=1, seg_rows=24,
            trunc=_tc("h1", "levels"), rows=rows, levels=(4, 2), intent="levels")
        add(f"A: {tag} top-K", "rows", one(mixed_strip, h), base=base, trunc=dict(truncate_method=T["topk"], feature_count_threshold=700),
            rows=rows, levels=(4, 2))

    # ---- B: a spill list longer than the placement grid covers
    grid3 = lambda: np.stack([dense_grid(1240, 480, 0), dense_grid(1240, 480, 1), dense_grid(1240, 480, 0, flip=True)])
    for b in range(3):
        add(f"B: grid 1240x480 batch of three, image {b}", "spill", grid3, base=GRID_KW, index=b, seg_rows=24, spill=True)
    add("B: grid 1240x480 batch of three, image 0, top-K 20000", "spill", grid3, base=GRID_KW, index=0, seg_rows=24,
        trunc=dict(truncate_method=T["topk"], feature_count_threshold=20000), spill=True, cut_inside_level=True)
    add(f"B: grid 1240x{GRID_SINGLE_H} one image", "spill", one(dense_grid, 1240, GRID_SINGLE_H, 0), base=GRID_KW, seg_rows=12, spill=True)

    # ---- C: top-K at the chunk edges
    for n in (4096, 4097, 8191, 8192):
        for d, tag in ((0, "n"), (-1, "n - 1"), (1, "n + 1")):
            add(f"C: n {n} K {tag}", "topk", one(tie_strip, n), base=TIE_BASE, trunc=_k_relative(d), n=n)
        add(f"C: n {n} K 1", "topk", one(tie_strip, n), base=TIE_BASE, trunc=dict(truncate_method=T["topk"], feature_count_threshold=1), n=n)
    for where, chunk in (("chunk 0", 0), ("end of chunk 0", 0), ("first of chunk 1", 1), ("chunk 1", 1), ("whole run", 1)):
        add(f"C: n 8192 cut in {where}", "topk", one(tie_strip, 8192), base=TIE_BASE, trunc=_tie_need(where), n=8192, where=where, chunk=chunk)
    add("C: n 12600 cut in chunk 2", "topk", one(tie_strip, 12600), base=TIE_BASE, trunc=_tie_need("chunk 2"), n=12600, where="chunk 2", chunk=2)
    add("C: weak band between strong ones", "topk", lambda: weak_strip()[None], base=TIE_BASE, trunc=_k_in_strong, idle_chunk=True)
    batch = lambda: np.stack([tie_strip(8192), np.full((256 + 8824, 64), 128, np.uint8), tie_strip(4097, pad_to=256 + 8824)])
    for b in range(3):
        add(f"C: batch of three, image {b}", "topk", batch, base=TIE_BASE, index=b, seg_rows=24,
            trunc=dict(truncate_method=T["topk"], feature_count_threshold=5000), n=(8192, 0, 4097)[b])

    # ---- D: feature scan
    for method in ("h1", "low"):
        add(f"D: one workgroup, {method} after the reshape", "scan", lambda: dense_strip()[None], base=dict(tex_max_dim=8192, max_orientation=2),
            trunc=_tc_second(method), passes=2, table_beyond_capacity=(method == "h1"))
    add("D: chunks, the last one empty", "scan", lambda: dense_strip()[None], base=dict(tex_max_dim=8192), chunks=15, empty_last=True)
    add("D: chunks, 15361 keypoints", "scan", lambda: dense_15361()[None], base=dict(tex_max_dim=8192), chunks=15, n=15361)
    return out


Result = namedtuple("Result", "raw keys desc geometry params counts")


def result_of(session, counts, b):
    keys, desc = session.fetch(b)
    return Result(session.rawlist(b), keys, desc, session.geometry(), session.params, counts)


class Mismatch(AssertionError):
    def __init__(self, stage, msg):
        super().__init__(f"[{stage}] {msg}")
        self.stage = stage


def _need(cond, stage, msg):
    if not cond:
        raise Mismatch(stage, msg() if callable(msg) else msg)


def check_case(run, case, wrong=None):
    """run(parameters) -> Result of image case.index of case.image() on a session with those parameters.  The list of the
    truncating session against the model (wrong: its switches) applied to the untruncated session's list; the reach the
    case is there for.  -> statistics.  Raises Mismatch for the model, AssertionError for the reach."""
    full = run(dict(case.base))
    raw = full.raw
    dog = int(full.params.dog_level_num) or 3
    plain = ListModel(full.params, full.geometry, case.seg_rows)
    _need(strictly_ordered(raw), "order", "the untruncated list is not strictly increasing in (level, row, col)")
    counts, first = orientation_counts(raw, full.keys, full.params)
    _need(int(counts.sum()) == len(full.keys) == full.counts[case.index], "table", "feature count of the untruncated session")
    trunc = case.trunc(plain, raw, counts) if callable(case.trunc) else case.trunc
    sel = run(dict(case.base, **trunc)) if trunc else full
    model = ListModel(sel.params, sel.geometry, case.seg_rows, **(wrong or {}))
    idx = model.select(raw)
    want = take(raw, idx)
    _need(len(sel.raw) == len(want), "list", lambda: f"{len(sel.raw)} entries, model {len(want)}")
    _need(sel.raw.tobytes() == want.tobytes(), "list",
          lambda: f"the list differs from the model's at entry {int(np.flatnonzero(sel.raw.view(np.uint8).reshape(-1, 32) != want.view(np.uint8).reshape(-1, 32))[0] // 32) if len(want) else 0}")
    _need(strictly_ordered(sel.raw), "order", "the list is not strictly increasing in (level, row, col)")
    hole = idx < 0
    lv = np.where(hole, 0, raw["level_index"][np.maximum(idx, 0)])
    cnt = np.where(hole, 0, counts[np.maximum(idx, 0)])
    table = model.features(lv, cnt)
    rows = np.array([first[idx[i]] + q for i, q in table], dtype=np.int64)
    _need(len(sel.keys) == len(rows) == sel.counts[case.index], "table", lambda: f"{len(sel.keys)} features (count {sel.counts[case.index]}), model {len(rows)}")
    _need(sel.keys.tobytes() == full.keys[rows].tobytes(), "table", "the keypoints are not those of the model's feature table, in its order")
    if sel.desc.size:
        _need(sel.desc.tobytes() == full.desc[rows].tobytes(), "table", "the descriptors are not those of the model's feature table")
    st = dict(n=len(raw), kept=len(sel.raw), features=len(sel.keys), full_features=len(full.keys), rows=list_rows(full.geometry, dog),
              level_counts=plain.level_counts(raw).tolist(), kept_level_counts=plain.level_counts(sel.raw).tolist(), trunc=trunc,
              orientations=np.bincount(counts).tolist(), capacity=planned_capacity(full.geometry, dog), nlev_per_octave=dog,
              first_pass_features=int(cnt.sum()))
    if trunc and trunc["truncate_method"] == T["topk"] and len(raw) >= trunc["feature_count_threshold"]:
        st["topk"] = model.topk_reach(topk_key(raw))
    st["spill"] = task_spill(raw, full.geometry, dog, case.seg_rows, [0])[0]
    return st


def check_reach(st, case):
    """The case reaches the seam it is there for (asserted from the untruncated list)."""
    r = case.reach
    if "rows" in r:
        assert st["rows"] == r["rows"], (st["rows"], r["rows"])
        assert (st["rows"] > REGISTER_ROWS) == (r["rows"] > REGISTER_ROWS)
        nlev, noct = r["levels"]
        filled = [i for i, c in enumerate(st["level_counts"]) if c]
        per_oct = st["nlev_per_octave"]
        assert len(filled) >= nlev and len({i // per_oct for i in filled}) >= noct, st["level_counts"]
    if "intent" in r:
        left = [i for i, c in enumerate(st["kept_level_counts"]) if c]
        gone = [i for i, c in enumerate(st["level_counts"]) if c and not st["kept_level_counts"][i]]
        assert intent_holds(r["intent"], left, gone, st["nlev_per_octave"]), (r["intent"], st["level_counts"], st["kept_level_counts"])
        assert all(st["kept_level_counts"][i] == st["level_counts"][i] for i in left)
    if r.get("spill"):
        assert st["spill"] > GRID_SPILL, st["spill"]
        assert st["n"] < st["capacity"], (st["n"], st["capacity"])
    if r.get("cut_inside_level"):
        cut = [k for k, c in zip(st["kept_level_counts"], st["level_counts"]) if 0 < k < c]
        assert cut, (st["kept_level_counts"], st["level_counts"])
    if "n" in r:
        assert st["n"] == r["n"], (st["n"], r["n"])
    if "chunk" in r:
        t = st["topk"]
        assert t["chunk"] == r["chunk"], t
        per = t["ties_in_chunk"]
        if r["where"] == "end of chunk 0":
            assert t["need"] == per[0] and t["ties_before_chunk"] == 0
        elif r["where"] == "first of chunk 1":
            assert t["need"] == per[0] + 1 == t["ties_before_chunk"] + 1
        elif r["where"] == "chunk 0":
            assert 0 < t["need"] < per[0]
        elif r["where"] == "chunk 1":
            assert t["ties_before_chunk"] == per[0] and per[0] + 100 < t["need"] < per[0] + per[1] - 100
        elif r["where"] == "chunk 2":
            # a whole chunk before the cut holds ties (and entries below the cut), no sure keep
            assert t["ties_before_chunk"] == per[0] + per[1] and per[1] > 3000 and t["sure_in_chunk"][1] == 0 and t["need"] > t["ties_before_chunk"] + 100
        elif r["where"] == "whole run":
            assert t["need"] == t["ties"] and t["sure"] + t["ties"] < st["n"]
    if r.get("idle_chunk"):
        t = st["topk"]
        idle = [c for c in range(1, len(t["ties_in_chunk"]) - 1) if t["ties_in_chunk"][c] == 0 and t["sure_in_chunk"][c] == 0]
        assert idle and t["chunk"] > idle[0] and 0 < t["need"] < t["ties"], t
    if "passes" in r:
        assert st["kept"] > SCAN_PASS * (r["passes"] - 1), st["kept"]
        assert 0 < st["features"] < st["first_pass_features"], (st["features"], st["first_pass_features"])
        assert all(st["orientations"][k] > 0 for k in (1, 2, 3, 4)), st["orientations"]   # (no keypoint of these inputs has none)
    if r.get("table_beyond_capacity"):
        # the rule drops the LOWEST level after the reshape: the kept features lie at the far end of the feature table, and
        # the table of all of them is longer than the planned feature capacity while the kept ones alone would fit
        assert st["first_pass_features"] > st["capacity"] > st["features"], (st["first_pass_features"], st["capacity"], st["features"])
    if "chunks" in r:
        nchunk, clen, used = scan_chunks(st["n"], st["capacity"])
        assert nchunk == r["chunks"], (nchunk, st["capacity"])
        assert used < nchunk, (st["n"], nchunk, clen, used)
        if "n" in r:
            assert st["n"] == 1024 * nchunk + 1
