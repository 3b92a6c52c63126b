"""Inputs and an independent model for the matcher tests (a plain helper module, no tests in it).

Why: a score is dot * 2^-18, clamped at 1 before acos.  Uniformly random bytes give dot products of about 2 M, eight times
the clamp: best and second are both at distance 0 and nothing ever matches, whatever the thresholds.  The sets made here
behave like descriptors -- sparse heavy-tailed rows of L2 norm 490 < 512, so every dot product stays under the clamp and
every distance is positive, duplicates included -- with correspondences between the sets and with exact ties placed where
the matrix-core kernel (hessgpu_amd/csrc/hess_match.hip) changes tile, super tile, segment, lane half, wavefront and row
block.

  descriptor_rows / noisy     the generator
  pair_seg / single_plan / chunk_sps   the host's plan of hess_match.hip restated: which segment geometry a size yields
  tie_groups / make_set       placed ties
  single_pair / bank_sets     the cases the CPU and the GPU tests share
  Model / model_match         NumPy model of the reference's matcher, with switches that state the WRONG rules
"""
import functools

import numpy as np

CLAMP = 1 << 18                     # dot products at or above it are at distance 0
TILE, SUPER, ROWS = 32, 128, 256    # columns per MFMA tile and per staged super tile, rows per workgroup (MM_SUPER, MM_ROWS)
MAX_SPS = 15                        # super tiles per segment at most: 60 tiles share six key bits with "none" (MM_MAX_TILES / 4)
MATRIX_CORE_ABOVE = 3 << 20         # hess_matcher_match: n1 * n2 above it runs on the matrix cores, else the one-pass kernel
BANK_CHUNK = 64                     # pairs per launch of hess_matcher_match_pairs (MP_PAIRS)

# L2 norm of a generated row.  Below 512 by enough that a noisy copy (+-6 per byte, clipped at 0, which adds up to about
# 12 000 to a squared norm of 240 100) stays below it too: every dot product is then under the clamp
NORM = 490.0

BREV5 = np.array([int(format(c, "05b")[::-1], 2) for c in range(32)])

# (distmax, ratiomax): the reference's defaults; a looser pair; no distance gate with the plain "best < second" test, which
# rejects every tied row; no gate at all -- every row (column) with a positive best score is returned, ties included
THRESHOLDS = ((0.7, 0.8), (1.2, 0.95), (2.0, 1.0), (2.0, 2.0))
CONFIGS = tuple((dm, rm, mutual) for mutual in (True, False) for dm, rm in THRESHOLDS)


# ---- generator ------------------------------------------------------------------------------------------------------

def descriptor_rows(n, rng, norm=NORM, peaky_every=4):
    """[n, 128] u8, every row of L2 norm <= `norm`.  Two families: gamma(0.35) rows (sparse, heavy tailed: a few percent of
    the bytes are >= 128, the signed-byte bias of the matrix-core path) and, every `peaky_every`-th row, three components in
    240..255 at positions drawn from 16 hot dimensions -- two such rows often share one, so products of two large bytes are
    common -- over a gamma background that fills the norm.  Floored to bytes, which only lowers the norm."""
    x = rng.gamma(0.35, size=(n, 128))
    big = np.zeros((n, 128))
    hot = np.arange(5, 128, 8)                                            # 16 dimensions
    for i in range(0, n, peaky_every):
        big[i, rng.choice(hot, 3, replace=False)] = rng.randint(240, 256, size=3)
    x[big > 0] = 0.0
    rest = np.sqrt(np.maximum(norm * norm - (big * big).sum(1, keepdims=True), 0.0))
    x *= rest / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), 1e-9)
    return np.minimum(np.floor(x + big), 255).astype(np.uint8)


def noisy(s, rng, amp=6):
    return np.clip(s.astype(np.int32) + rng.randint(-amp, amp + 1, size=s.shape), 0, 255).astype(np.uint8)


# ---- the host's plan, restated (hess_match.hip: pair_seg, hess_matcher_match, chunk_sps) ------------------------------

def pair_seg(nsuper, sps):
    """Segments of a pair of `nsuper` super tiles when a segment may hold `sps`: -> (segments, super tiles per segment)."""
    nseg = -(-nsuper // sps)
    psps = -(-nsuper // nseg)
    return -(-nsuper // psps), psps


def single_plan(n1, n2):
    """hess_matcher_match above MATRIX_CORE_ABOVE: -> (row blocks, super tiles, segments, super tiles per segment)."""
    nrb, nsuper = -(-n1 // ROWS), -(-n2 // SUPER)
    target = 512 if nrb * nsuper >= 512 * 4 else 256
    nseg = min(max(-(-target // nrb), 1), nsuper)
    nseg, psps = pair_seg(nsuper, min(-(-nsuper // nseg), MAX_SPS))
    return nrb, nsuper, nseg, psps


def chunk_sps(sizes):
    """Super tiles per segment at most, for one match_pairs chunk of pairs [(n1, n2), ...]."""
    work = sum(-(-a // ROWS) * -(-b // SUPER) for a, b in sizes if a and b)
    target = 512 if work >= 512 * 4 else 256
    return min(max(-(-work // target), 1), MAX_SPS)


# ---- placed ties ----------------------------------------------------------------------------------------------------

def tie_groups(n, sps_list):
    """Positions of exact duplicates in a set of n rows: {name: (positions...)}; every name gets one descriptor of its own,
    the same in every set of a case, so in a pair (A, B) the rows of A that hold it tie on the columns of B that hold it
    (row decision: the reference's tree picks the smallest bit-reversed class j % 32, then the lowest j) and those columns
    tie on those rows (column decision: the lowest row).  A set serves in both roles, so every group is both.
    sps_list: the super tiles per segment the set meets as set 2; the groups that depend on it are placed for each.  A
    group that does not fit into n rows or meets an occupied position is left out (tie_groups is deterministic)."""
    want = [
        # set 2, one 32-column tile (tile 1), classes whose numeric and bit-reversed orders disagree: class 2 (bit-reversed
        # 8) beats class 1 (16); class 16 (1) beats class 3 (24) -- the merge of a row's 32 classes at a segment's end
        ("tile_classes_1_2", (TILE + 1, TILE + 2)),
        ("tile_classes_3_16", (TILE + 3, TILE + 16)),
        # same class in two tiles of one super tile (0 and 3), and of two super tiles: the earlier tile, kept by the packed
        # key's tile index (62 - tile in its low six bits)
        ("class_5_tiles_1_3", (TILE + 5, 3 * TILE + 5)),
        # first and last column: class 0 against the last class of the set (which is in the ragged last tile)
        ("first_last_column", (0, n - 1)),
        # set 1, rows 16 apart (the two lane halves of one 32-row MFMA block), 32 apart (the two blocks of a wavefront), 64
        # apart (two wavefronts), 256 apart (two workgroups, merged by match_col_block), and (last row, early row): the
        # lowest row must win the column decision
        ("rows_16_apart", (10, 26)),
        ("rows_32_apart", (11, 43)),
        ("rows_64_apart", (12, 76)),
        ("rows_256_apart", (13, 269)),
        ("last_row_early_row", (14, n - 2)),
    ]
    nsuper = -(-n // SUPER)
    for nseg, psps in sorted({pair_seg(nsuper, min(sps, nsuper)) for sps in sps_list} if n else ()):
        S = psps * SUPER                               # columns per segment
        last_seg = (nseg - 1) * S                      # first column of the last segment
        last_tile = (n - 1) // TILE * TILE             # first column of the last tile that holds a descriptor
        t = f"_sps{psps}"
        want += [
            # same class in tile 1 of segments 0 and 1: match_finish_kernel keeps the lower column
            ("class_6_two_segments" + t, (TILE + 6, S + TILE + 6)),
            # class 9 (bit-reversed 18) in segment 0, class 10 (bit-reversed 10) in segment 1: the LATER column wins, which
            # match_finish_kernel has to decide from the classes of two segments' states
            ("classes_9_10_two_segments" + t, (TILE + 9, S + TILE + 10)),
            # three copies: classes 1, 2 in segment 0 and class 3 in segment 1 -- class 2 wins, second == best
            ("three_copies" + t, (2 * TILE + 1, 2 * TILE + 2, S + 2 * TILE + 3)),
            # first and last tile of segment 0 (tile index 0 and 4 psps - 1: at sps 15 that is 59, the largest the key
            # holds): classes 17 (bit-reversed 17) and 18 (9) -- the last tile's column wins; class 19 in both: the first
            ("segment_first_last_tile" + t, (17, S - TILE + 18)),
            ("segment_first_last_tile_same_class" + t, (19, S - TILE + 19)),
            # the same in the last segment, whose last tile is ragged: class 1 in its first tile, class 2 in the set's last
            ("last_segment_first_last_tile" + t, (last_seg + 1, last_tile + 2)),
        ]
    out, used = {}, set()
    for name, pos in want:
        if min(pos) < 0 or max(pos) >= n or len(set(pos)) < len(pos) or used & set(pos):
            continue
        out[name] = pos
        used |= set(pos)
    return out


N_FIXED_GROUPS, N_SPS_GROUPS = 9, 6
MAX_TIE_ROWS = N_FIXED_GROUPS + MAX_SPS * N_SPS_GROUPS
_FIXED = ("tile_classes_1_2", "tile_classes_3_16", "class_5_tiles_1_3", "first_last_column", "rows_16_apart",
          "rows_32_apart", "rows_64_apart", "rows_256_apart", "last_row_early_row")
_PER_SPS = ("class_6_two_segments", "classes_9_10_two_segments", "three_copies", "segment_first_last_tile",
            "segment_first_last_tile_same_class", "last_segment_first_last_tile")


def tie_index(name):
    """The descriptor of a group: one per name, the same in every set of a case."""
    if name in _FIXED:
        return _FIXED.index(name)
    stem, sps = name.rsplit("_sps", 1)
    return N_FIXED_GROUPS + (int(sps) - 1) * N_SPS_GROUPS + _PER_SPS.index(stem)


def make_set(n, pool, ties, rng, sps_list=(1,)):
    """A set of n rows: two thirds are noisy copies (+-6) of the first rows of `pool` (so any two sets of a case correspond in
    two thirds of the smaller one), the rest are fresh rows; all at random positions.  Then the tie groups (ties[k] for the
    group tie_index(name), exact) and, from 64 rows on, one all-zero row (score 0 is never a maximum, index -1)."""
    groups = tie_groups(n, sps_list)
    taken = sorted(p for pos in groups.values() for p in pos)
    free = np.setdiff1d(np.arange(n), taken)
    if n >= 64:
        taken.append(int(free[free >= 40][0]))     # the all-zero row
        free = np.setdiff1d(free, taken)
    common = (2 * n + 2) // 3
    rows = np.concatenate([noisy(pool[:common], rng), descriptor_rows(n - common, rng)])
    s = np.zeros((n, 128), np.uint8)
    s[rng.permutation(free)] = rows[:len(free)]     # (the placed rows take the room of the last fresh ones)
    for name, pos in groups.items():
        s[list(pos)] = ties[tie_index(name)]
    return s


def _case_material(seed, nmax):
    rng = np.random.RandomState(seed)
    pool = descriptor_rows((2 * nmax + 2) // 3, rng)
    ties = descriptor_rows(MAX_TIE_ROWS, rng)
    return rng, pool, ties


# ---- the cases ------------------------------------------------------------------------------------------------------

# Single pairs on the matrix cores (n1 * n2 > 3 Mi), with the geometry single_plan gives (row blocks x segments of
# super tiles; test_matcher_cases.py asserts these figures):
MATRIX_CORE_SIZES = (
    (2049, 2081),    # 9 row blocks (the last holds 1 row), 17 super tiles (the last holds 33 columns), 17 segments of 1
    (255, 12337),    # 1 ragged row block, 97 segments of 1 super tile, the last holds 49 columns
    (257, 12289),    # 2 row blocks (256 + 1), 97 segments of 1, the last super tile holds 1 column
    (12001, 263),    # tall: 47 row blocks, 3 segments of 1 super tile; the column partials of 47 blocks meet in match_col_block
    (300, 33000),    # wide: 2 row blocks, 258 super tiles in 86 segments of 3 (12 tiles per segment)
)
# The same generator under the threshold (match_dot_kernel / match_row_kernel), and one pair of sets straddling it: 1536 x
# 2048 is exactly 3 Mi products and stays on the small path, one row more goes to the matrix cores.
SMALL_PATH_SIZES = ((1000, 877), (1536, 2048))
STRADDLE = ((1536, 2048), (1537, 2048))


@functools.lru_cache(maxsize=None)
def single_pair(n1, n2, seed=5):
    """-> (set 1, set 2) with correspondences and placed ties for the geometry of its size."""
    rng, pool, ties = _case_material(seed, max(n1, n2))
    sps = single_plan(n1, n2)[3] if n1 * n2 > MATRIX_CORE_ABOVE else 1
    return make_set(n1, pool, ties, rng, (1, sps)), make_set(n2, pool, ties, rng, (1, sps))


@functools.lru_cache(maxsize=None)
def straddle_sets(seed=6):
    """One set of 1537 rows and one of 2048: rows [:1536] against the second stay on the small path, all 1537 do not."""
    rng, pool, ties = _case_material(seed, 2048)
    return make_set(1537, pool, ties, rng), make_set(2048, pool, ties, rng)


# The bank: sizes around the 256-row block; 1500 / 3100 / 3825 rows are 12 / 25 / 30 super tiles as set 2.  A chunk of 64
# pairs of these three reaches the cap of 15 super tiles per segment: pair_seg(25, 15) = 2 segments of 13 (tiles 0..51),
# pair_seg(30, 15) = 2 of 15 (tiles 0..59; 3825 = 2 * 1920 - 15 rows, so tile 59 of BOTH segments holds descriptors).
BANK_SIZES = (0, 1, 31, 255, 256, 257, 1500, 3100, 3825)
BANK_ZERO_SET = len(BANK_SIZES)            # index of the all-zero set (300 rows): the one case that must give no match
BANK_BIG = (6, 7, 8)
BANK_MAX_SIFT = 3900


@functools.lru_cache(maxsize=None)
def bank_sets(seed=7):
    rng, pool, ties = _case_material(seed, max(BANK_SIZES))
    # as set 2 a bank set meets one super tile per segment (single pairs, small chunks), the all-pairs chunks' 2 and 6 and the cap
    sets = [make_set(n, pool, ties, rng, (1, 2, 6, MAX_SPS)) if n else np.zeros((0, 128), np.uint8) for n in BANK_SIZES]
    return sets + [np.zeros((300, 128), np.uint8)]


def bank_all_pairs():
    n = len(BANK_SIZES) + 1
    return np.array([(a, b) for a in range(n) for b in range(n)], np.int32)      # (a, a) included


def bank_big_chunk_pairs():
    """64 pairs of the three large sets in one chunk: its work (16 000 workgroup-super-tiles) puts chunk_sps at the cap."""
    nine = [(a, b) for a in BANK_BIG for b in BANK_BIG]
    return np.array([nine[k % 9] for k in range(BANK_CHUNK)], np.int32)


# ---- the model ------------------------------------------------------------------------------------------------------

def _decide(best, second, idx, distmax, ratiomax):
    """The reference's test, as RowMatch_Kernel / ColMatch_Kernel write it: score in float, acos in double, compared in float."""
    k = np.float32(0.000003814697265625)
    dist = np.arccos(np.minimum((best.astype(np.float32) * k).astype(np.float64), 1.0)).astype(np.float32)
    distn = np.arccos(np.minimum((second.astype(np.float32) * k).astype(np.float64), 1.0)).astype(np.float32)
    return np.where((dist < np.float32(distmax)) & (dist < distn * np.float32(ratiomax)), idx, -1)


def _top2(m):
    """Per row: the largest and the second largest entry counting duplicates, both at least 0."""
    p = np.concatenate([m, np.zeros((m.shape[0], 2), m.dtype)], 1)
    p = -np.partition(-p, 1, axis=1)[:, :2]
    return p[:, 0], p[:, 1]


class Model:
    """The matcher of the reference as a rule, not as its loops: all dot products; per row the best score (> 0, else index
    -1) at the smallest (bit-reversed class j % 32, j) among the maxima, per column at the lowest row; second = the second
    largest counting duplicates, floor 0; the acos decision; (i, j) in row order, mutual or not, the first max_match.

    row_rule "class" (lowest class, then lowest j) and "col" (lowest j), col_rule "high" (highest row) and
    second_counts_duplicates=False state WRONG rules with the same code: the tests use them to show that the inputs tell the
    rules apart."""

    def __init__(self, d1, d2):
        # float64 products through BLAS are exact here: every sum is below 128 * 255^2 < 2^24
        self.dot = np.rint(d1.astype(np.float64) @ d2.astype(np.float64).T).astype(np.int64)
        self.n1, self.n2 = self.dot.shape

    def _side(self, m, prio, dups):
        best, second = _top2(m)
        if not dups:
            second = np.where(m < best[:, None], m, 0).max(1, initial=0)
        cand = np.where(m == best[:, None], prio[None, :], np.iinfo(np.int64).max)
        return best, second, np.where(best > 0, cand.argmin(1), -1)

    def match(self, distmax=0.7, ratiomax=0.8, mutual=True, max_match=4096, row_rule="brev", col_rule="low",
              second_counts_duplicates=True):
        if self.n1 == 0 or self.n2 == 0:
            return np.zeros((0, 2), np.int32)
        j, i = np.arange(self.n2), np.arange(self.n1)
        prio = {"brev": BREV5[j % 32] * self.n2 + j, "class": (j % 32) * self.n2 + j, "col": j}[row_rule]
        rowm = _decide(*self._side(self.dot, prio, second_counts_duplicates), distmax, ratiomax)
        keep = rowm >= 0
        if mutual:
            colm = _decide(*self._side(self.dot.T, {"low": i, "high": -i}[col_rule], second_counts_duplicates), distmax,
                           ratiomax)
            keep &= colm[np.maximum(rowm, 0)] == i
        rows = np.flatnonzero(keep)[:max_match]
        return np.stack([rows, rowm[rows]], 1).astype(np.int32)


def model_match(d1, d2, **kw):
    return Model(d1, d2).match(**kw)


def first_difference(ref, got):
    """What a failing comparison prints: the first row where two match lists part."""
    r, g = dict(map(tuple, ref)), dict(map(tuple, got))
    for i in sorted(set(r) | set(g)):
        if r.get(i) != g.get(i):
            return f"row {i}: expected column {r.get(i)}, got {g.get(i)} ({len(ref)} expected matches, {len(got)} returned)"
    return f"same rows and columns, {len(ref)} expected matches, {len(got)} returned"
