"""A plain host reference of what the set-up unit hands to every later pass (tsem_rowstats and tsem_set_model of
telescope_amd/csrc/tsem_setup.hip: k_rowstats<G>, k_pisum_finish, k_colsig<G>, the twin search), and the seeded matrices that
tests/test_setup_reference.py (CPU: every input is fair) and tests/test_gpu_setup_products.py (GPU: the kernels against this file)
share.  numpy, math.fsum and Python integers only; nothing here touches the engine.

 * Y, the row code and w: Y = (len > 1), w = lut[largest code of the row], 0 for an empty row (model.py:679, 690).
 * stats3: W_tot and W_amb as math.fsum, w_max.
 * pisum0 per column, three ways: the exact sum as a Python integer in units of 2^-1074 (and, correctly rounded, by math.fsum); the
   emulation of the device's level split — every unique row's Q cut on PIS_LEVELS grids PIS_W bits apart with the kernel's own two
   operations, (r + mm) - mm and r -= piece, the grid top from frexp(lut[-1]), every level summed exactly (as integer multiples of its
   grid), the levels added from small to large in fp64; and what the split leaves over.
 * the column signature: the entry count and the sum modulo 2^32 of the 32-bit entry hash.  NOTE what the device's 64-bit value is:
   a sum over workgroups of (sums modulo 2^32), so only its LOW 32 BITS are a function of the matrix — the high half counts how
   often a workgroup's sum wrapped, which depends on how the rows fell to the workgroups.  Tests compare `hsh & 0xFFFFFFFF` with
   the model, and the classes of the full 64-bit value with the true classes.
 * the true twin classes straight from the CSC: same rows, same codes; representative = smallest index; count-0 columns alone.
 * the counts behind the shortcuts of tsem_reassign and the row-length histogram that picks the kernels.

NOT covered: a level sum of 2^26 pieces (67M unique rows in one column: where the exactness of a level ends) — not a few-second
test; the blocked layout (tests/test_gpu_em_pass_exact.py holds the passes that read it to an exact reference); tsem_generate.

The bounds, none of them tuned on a kernel's output:
 * W_tot, W_amb: (N - 1) 2^-53 relative — N non-negative numbers added in ANY order, each addition within 2^-53 of its result.
 * pisum0 inside the levels' range: (PIS_LEVELS - 1) 2^-53 relative.  The levels are exact; the partial sums t_k of k_pisum_finish
   (levels k .. 8) are sums of the rows' remainders after level k - 1, each at most its Q in magnitude (round to nearest on a
   grid: a Q below half a step stays whole, any other is off by at most half a step <= Q), so |t_k| <= the exact sum and each of
   the 8 additions errs by at most 2^-53 of it.
 * pisum0 past the range (the contract of include/telescope_em.h): (n_j + PIS_LEVELS) 2^-53 relative, n_j unique rows in column j —
   n_j remainders (each at most its Q) added by fp64 atomics in any order, then the 9 additions of k_pisum_finish.
"""
import math

import numpy as np
import scipy.sparse as sp

U = 2.0 ** -53
PIS_LEVELS, PIS_W = 9, 26                         # tsem_setup.hip
# floor(log2(largest)) - floor(log2(smallest positive)) of a table that the levels take whole: the grids reach 9 x 26 bits below the
# power of two above the last entry, a Q's last mantissa bit lies 52 below its leading one
PIS_EXACT_SPAN = PIS_LEVELS * PIS_W - 53          # 181
SIG_WIN = 18432                                   # columns per sweep of k_colsig
GOLDEN, M1, M2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
M64, M32 = (1 << 64) - 1, (1 << 32) - 1
LEN_STEPS = (8, 16, 32, 64, 128, 256)             # the row-length histogram of k_rowstats: rows LONGER than these
# The kernel variants (sixteen entries per lane, G lanes per row), stated once:
#  k_rowstats<G>: the smallest G of 1, 2, 4, 8 with 1.5 x mean row length <= 16 G, else 16 (tsem_rowstats);
#  k_colsig<G>:   the smallest G of 1, 2, 4, 8, 16 such that at most LONG_SHARE of the rows are longer than 16 G, else 16.
LANES = (1, 2, 4, 8, 16)
LONG_SHARE = 0.005


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def row_outputs(raw, lut):
    """(Y uint8[N], code[N], w[N])"""
    lens = np.diff(raw.indptr)
    code = np.zeros(raw.shape[0], dtype=np.int64)
    full = lens > 0
    if raw.nnz:
        code[full] = np.maximum.reduceat(raw.data.astype(np.int64), raw.indptr[:-1][full])
    w = np.where(full, np.asarray(lut)[code], 0.0)
    return (lens > 1).astype(np.uint8), code, w


def stats3(raw, lut):
    """(W_tot, W_amb, w_max): the first two correctly rounded"""
    Y, _, w = row_outputs(raw, lut)
    return math.fsum(w.tolist()), math.fsum(w[Y == 1].tolist()), float(w.max(initial=0.0))


def sum_fraction(got, exact, n):
    """|got - exact| as a fraction of (n - 1) 2^-53 exact: the bound for any order of n non-negative additions"""
    if exact == 0.0:
        return 0.0 if got == 0.0 else np.inf
    return abs(got - exact) / (max(n - 1, 1) * U * exact)


# ---- pisum0 -------------------------------------------------------------------------------------------------------------------------
def units(x):
    """a finite double as a Python integer in units of 2^-1074: exact"""
    num, den = float(x).as_integer_ratio()
    return num * ((1 << 1074) // den)


def unique_rows(raw):
    """(column, code) of the rows with exactly one stored entry, in row order"""
    at = raw.indptr[:-1][np.diff(raw.indptr) == 1]
    return raw.indices[at].astype(np.int64), raw.data[at].astype(np.int64)


def level_plan(lut):
    """[(lv, mm, grid exponent)] of the levels the kernel runs for this table: mm = 1.5 x 2^(e + 26 - 26 lv) is the rounding constant
    of level lv, its pieces are multiples of 2^(e - 26 (lv + 1)); e from frexp of the LAST entry (1.0 for a table ending in 0)"""
    e = math.frexp(float(lut[-1]) if lut[-1] > 0 else 1.0)[1]
    if e + 1023 + 52 - PIS_W > 2046:               # the top level's constant would overflow: no levels at all
        return []
    plan = []
    for lv in range(PIS_LEVELS):
        field = e + 1023 - PIS_W * lv + 52 - PIS_W   # the exponent field of mm
        if field < 1:                              # below the normal range: the loop ends
            break
        plan.append((lv, math.ldexp(1.5, field - 1023), e - PIS_W * (lv + 1)))
    return plan


class Pisum0(object):
    """exact_units[K] (Python integers, units of 2^-1074), exact[K] (math.fsum), emulated[K] (the level split WITHOUT what it leaves
    over: what the kernel gave before it kept the remainder, and what it gives where nothing is left), left[K] (the sum of the
    remainders' magnitudes: 0 inside the levels' range), n[K] unique rows per column, positive[K]: some unique row has Q > 0"""

    def __init__(self, raw, lut):
        K = raw.shape[1]
        lut = np.asarray(lut, dtype=np.float64)
        col, code = unique_rows(raw)
        q = lut[code]
        self.n = np.bincount(col, minlength=K)
        order = np.argsort(col, kind='stable')
        start = np.concatenate([[0], np.cumsum(self.n)])
        self.exact = np.zeros(K)
        self.exact_units = [0] * K
        qs = q[order].tolist()
        for j in np.flatnonzero(self.n):
            part = qs[start[j]:start[j + 1]]
            self.exact[j] = math.fsum(part)
            self.exact_units[j] = sum(units(x) for x in part)
        self.positive = np.array([x > 0 for x in self.exact_units], dtype=bool)
        r = q.copy()
        levels = np.zeros((PIS_LEVELS, K))
        self.level_pieces = 0
        for lv, mm, g in level_plan(lut):
            piece = (r + mm) - mm
            r = r - piece
            k = np.rint(np.ldexp(piece, -g)).astype(np.int64)          # exact: a piece is a multiple of 2^g below 2^(g + 27)
            assert np.array_equal(np.ldexp(k.astype(np.float64), g), piece)
            tot = np.zeros(K, dtype=np.int64)
            np.add.at(tot, col, k)
            assert np.abs(tot).max(initial=0) < 1 << 53                # the level's sum is a double
            levels[lv] = np.ldexp(tot.astype(np.float64), g)
            self.level_pieces = max(self.level_pieces, int(np.bincount(col[piece != 0], minlength=K).max(initial=0)))
        t = np.zeros(K)
        for lv in range(PIS_LEVELS - 1, -1, -1):
            t = t + levels[lv]
        self.emulated = t
        self.left = np.zeros(K)
        np.add.at(self.left, col, np.abs(r))
        self.remainder_exceeds_q = bool(np.any(np.abs(r) > q))
        self._levels, self._col, self._r = levels, col, r

    def kept(self, reverse=False):
        """the split WITH what it leaves over, as the kernel keeps it: the remainders added in fp64 one after the other (in row
        order, or in the reverse: two of the orders the atomics may take), then the levels from small to large"""
        t = np.zeros(len(self.n))
        o = slice(None, None, -1) if reverse else slice(None)
        np.add.at(t, self._col[o], self._r[o])                         # (unbuffered: sequential fp64 additions)
        for lv in range(PIS_LEVELS - 1, -1, -1):
            t = t + self._levels[lv]
        return t

    def fraction(self, got, j, bound_terms):
        """|got_j - exact_j| as a fraction of bound_terms x 2^-53 exact_j, in exact integer arithmetic"""
        ex = self.exact_units[j]
        if ex == 0:
            return 0.0 if got[j] == 0.0 else np.inf
        return float(abs(units(got[j]) - ex) * (1 << 53) / (bound_terms * ex))

    def worst(self, got, extra_terms=False):
        """the largest fraction over the columns: of (PIS_LEVELS - 1) 2^-53, or with extra_terms of (n_j + PIS_LEVELS) 2^-53"""
        top, at = 0.0, -1
        for j in np.flatnonzero(self.n):
            f = self.fraction(got, j, int(self.n[j]) + PIS_LEVELS if extra_terms else PIS_LEVELS - 1)
            if f > top:
                top, at = f, int(j)
        return top, at


def table_span(lut):
    """floor(log2(largest)) - floor(log2(smallest positive entry)); the levels take a table whole while this is <= PIS_EXACT_SPAN"""
    pos = np.asarray(lut)[np.asarray(lut) > 0]
    return (math.frexp(float(pos.max()))[1] - math.frexp(float(pos.min()))[1]) if len(pos) else 0


def table_is_fair(lut):
    """finite, non-negative, non-decreasing: what include/telescope_em.h asks of a caller's table"""
    lut = np.asarray(lut)
    return bool(np.all(np.isfinite(lut)) and np.all(lut >= 0) and np.all(np.diff(lut) >= 0))


# ---- column signatures -----------------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * M1) & M64
    z = ((z ^ (z >> 27)) * M2) & M64
    return z ^ (z >> 31)


def row_hash(global_row):
    return mix64(0x7715 ^ ((global_row * GOLDEN) & M64)) >> 32


def entry_hash(hrow, code):
    hv = hrow ^ ((code * 0x9E3779B1) & M32)
    hv ^= hv >> 15
    hv = (hv * 0x85EBCA77) & M32
    return hv ^ (hv >> 13)


def signature(raw, row_offset=0):
    """(cnt uint64[K], h32 uint64[K]): stored entries per column, and the sum modulo 2^32 of the entry hashes — in numpy, with the
    scalar functions above as the statement of the hash (tests/test_setup_reference.py holds the two together)"""
    K = raw.shape[1]
    rows = (np.arange(raw.shape[0], dtype=np.uint64) + np.uint64(row_offset))
    with np.errstate(over='ignore'):
        z = np.uint64(0x7715) ^ (rows * np.uint64(GOLDEN))
        z = z + np.uint64(GOLDEN)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
        z = z ^ (z >> np.uint64(31))
        hrow = np.repeat(z >> np.uint64(32), np.diff(raw.indptr))
        m32 = np.uint64(M32)
        hv = hrow ^ ((raw.data.astype(np.uint64) * np.uint64(0x9E3779B1)) & m32)
        hv = hv ^ (hv >> np.uint64(15))
        hv = (hv * np.uint64(0x85EBCA77)) & m32
        hv = hv ^ (hv >> np.uint64(13))
        h = np.zeros(K, dtype=np.uint64)
        np.add.at(h, raw.indices, hv)
    return np.bincount(raw.indices, minlength=K).astype(np.uint64), h & m32


def true_twins(raw):
    """(rep int64[K], twin columns): rep[j] = the smallest column with j's rows and codes; a column without entries stands alone"""
    csc = sp.csc_matrix(raw)
    csc.sort_indices()
    K = raw.shape[1]
    # (scipy drops nothing here: stored zeros stay stored)
    assert csc.nnz == raw.nnz
    rep = np.arange(K, dtype=np.int64)
    seen = {}
    for j in range(K):
        a, b = csc.indptr[j], csc.indptr[j + 1]
        if a == b:
            continue
        key = (csc.indices[a:b].astype(np.int64).tobytes(), csc.data[a:b].astype(np.int64).tobytes())
        rep[j] = seen.setdefault(key, j)
    size = np.bincount(rep, minlength=K)
    return rep, int(size[size > 1].sum())


def colliding_columns(raw, row_offset=0):
    """pairs of columns that are NOT twins, hold equally many entries and share the modelled 32-bit hash: none, for a fair matrix"""
    cnt, h32 = signature(raw, row_offset)
    rep, _ = true_twins(raw)
    seen, bad = {}, []
    for j in np.flatnonzero(cnt):
        key = (int(cnt[j]), int(h32[j]))
        if key in seen and rep[seen[key]] != rep[j]:
            bad.append((seen[key], int(j)))
        seen.setdefault(key, int(j))
    return bad


# ---- counts -----------------------------------------------------------------------------------------------------------------------------
class Counts(object):
    """the numbers behind layout_info and the shortcuts of tsem_reassign"""

    def __init__(self, raw, lut):
        K = raw.shape[1]
        lens = np.diff(raw.indptr)
        self.N_amb, self.N_uni = int((lens > 1).sum()), int((lens == 1).sum())
        self.nnz_amb = int(lens[lens > 1].sum())
        self.len_gt = [int((lens > s).sum()) for s in LEN_STEPS]
        self.has_zero = bool(np.any(raw.data == 0))
        col, code = unique_rows(raw)
        self.unique = np.bincount(col[code != 0], minlength=K).astype(np.float64)     # reassign('unique')
        self.entries = np.bincount(raw.indices, minlength=K).astype(np.float64)       # reassign('all', initial) without a stored 0
        # ... and what the row pass counts: the entries with a positive Q (every row here that stores a 0 also stores a positive score)
        self.positive_entries = np.bincount(raw.indices[np.asarray(lut)[raw.data] > 0], minlength=K).astype(np.float64)


def rowstats_lanes(raw):
    mean = raw.nnz / float(raw.shape[0])
    for g in LANES[:-1]:
        if mean * 1.5 <= 16 * g:
            return g
    return 16


def colsig_lanes(raw):
    lens = np.diff(raw.indptr)
    for g in LANES:
        if float((lens > 16 * g).sum()) <= LONG_SHARE * float(raw.shape[0]):
            return g
    return 16


# ---- matrices -------------------------------------------------------------------------------------------------------------------------
REF_TABLES = (255, 400, 65535)                    # largest scores of the reference's tables used here (likelihood.score_lut)
BIG = 250                                         # the largest code of every matrix on score_lut(255); all other codes stay below SMALL
SMALL = 200


def table(max_score):
    from telescope_amd.likelihood import score_lut
    return score_lut(max_score)


def wide_table(n=256):
    """a caller's table PAST the levels' range: non-decreasing, lut[0] = 0, 2^-520 ... 2^459 — a span of 979 binades"""
    t = np.ldexp(1.0 + np.arange(n) / 1024.0, np.linspace(-520, 459, n).astype(int))
    t[0] = 0.0
    return t


def huge_table(n=256):
    """a caller's table whose last entry is past 2^997, where the top level's rounding constant would overflow: no levels, every Q is
    a remainder; 2^20 ... 2^1000"""
    t = np.ldexp(1.0 + np.arange(n) / 1024.0, np.linspace(20, 1000, n).astype(int))
    t[0] = 0.0
    return t


def special_lengths(G):
    return sorted(set([0, 1, 2, 15, 16, 17, 16 * G - 1, 16 * G, 16 * G + 1, 32 * G, 32 * G + 1, 48 * G + 5]))


class Built(object):
    """raw (CSR with sorted column ids; a stored 0 stays stored) and what the builder planted: the columns of every twin case, the
    rows S that carry them, the rows behind a row of length 1 mod 16"""


UNIQUE_COLS = 24


def _assemble(lens, K, plan, first_code, rng, hi=SMALL):
    """lens[i] entries in row i: the planted (row -> [(column, code)]) entries first, the rest in random other columns with codes in
    [1, hi) — a single-entry row in one of UNIQUE_COLS columns, so that a column of pisum0 sums several rows —; first_code: row -> the
    code of the row's FIRST stored entry"""
    planted = sorted(set(c for ents in plan.values() for c, _ in ents))
    reserved = np.zeros(K, dtype=bool)
    reserved[planted] = True
    free = np.flatnonzero(~reserved)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.empty(indptr[-1], dtype=np.int32)
    data = np.empty(indptr[-1], dtype=np.uint16)
    for i, n in enumerate(lens):
        ents = plan.get(i, [])
        assert len(ents) <= n, (i, n, len(ents))
        pool = free[10:10 + UNIQUE_COLS] if n == 1 else free
        cols = np.concatenate([[c for c, _ in ents], rng.choice(pool, n - len(ents), replace=False)]).astype(np.int64)
        codes = np.concatenate([[v for _, v in ents], rng.integers(1, hi, n - len(ents))]).astype(np.int64)
        o = np.argsort(cols)
        cols, codes = cols[o], codes[o]
        if i in first_code:
            assert not reserved[cols[0]]
            codes[0] = first_code[i]
        indices[indptr[i]:indptr[i + 1]] = cols
        data[indptr[i]:indptr[i + 1]] = codes
    raw = sp.csr_matrix((data, indices, indptr), shape=(len(lens), K))
    assert raw.has_sorted_indices and raw.nnz == indptr[-1]
    return raw


def _twin_plan(S, cols, rng, hi=SMALL):
    """the twin cases on the rows S (>= 21 of them, ascending), columns by name:
    pair (2 columns): rows S[0:10], the same codes;  triple (3): rows S[5:20], the same codes;
    score (2): rows S[0:10], the same codes but one;  row (2): rows S[0:10] against S[0:9] + S[10], the same codes in order
    -> {row: [(column, code)]}"""
    plan = {}

    def put(col, rows, codes):
        for r, v in zip(rows, codes):
            plan.setdefault(int(r), []).append((int(col), int(v)))
    if 'pair' in cols:
        v = rng.integers(1, hi, 10)
        for c in cols['pair']:
            put(c, S[0:10], v)
    if 'triple' in cols:
        v = rng.integers(1, hi, 15)
        for c in cols['triple']:
            put(c, S[5:20], v)
    if 'score' in cols:
        v = rng.integers(1, hi - 1, 10)
        w = v.copy()
        w[4] += 1
        put(cols['score'][0], S[0:10], v)
        put(cols['score'][1], S[0:10], w)
    if 'row' in cols:
        v = rng.integers(1, hi, 10)
        put(cols['row'][0], S[0:10], v)
        put(cols['row'][1], list(S[0:9]) + [S[10]], v)
    return plan


def _place(lens_filler, specials, rng, pairs_after):
    """row lengths: the fillers and the special lengths in random order, and behind one row of each length in pairs_after
    a row of 3 entries (the row whose FIRST entry gets the marked code); the matrix ends on a row of 17 entries.
    -> (lens, [rows behind a row of length 1 mod 16])"""
    body = [(int(n), None) for n in lens_filler] + [(int(n), 'special') for n in specials]
    order = rng.permutation(len(body))
    lens, behind = [], []
    todo = list(pairs_after)
    for t in order:
        n, tag = body[t]
        lens.append(n)
        if tag == 'special' and n in todo:
            todo.remove(n)
            behind.append(len(lens))
            lens.append(3)
    assert not todo, todo
    lens.append(17)                                  # the matrix's last row ends on a length of 1 mod 16 too: the padding follows
    return np.array(lens, dtype=np.int64), behind


TWIN_COLS = {'pair': (3, 4), 'triple': (100, 101, 700), 'score': (50, 51), 'row': (60, 61)}
EMPTY_COLS = (7, 500, 1199)
K_SMALL = 1200


def _finish(raw, lens, behind, S, cols, empty, max_score):
    b = Built()
    b.raw, b.behind, b.S, b.cols, b.empty, b.max_score = raw, behind, np.asarray(S), cols, empty, max_score
    assert max_score in REF_TABLES
    b.lut = table(max_score)
    assert np.array_equal(np.diff(raw.indptr), lens)
    return b


def _small_matrix(lens, behind, rng, first, max_score=255, K=K_SMALL):
    lens = np.asarray(lens)
    ok = np.ones(len(lens), dtype=bool)
    ok[behind] = False
    ok[np.asarray(behind) - 1] = False
    S = np.flatnonzero((lens >= 12) & (lens <= 40) & ok)
    if len(S) < 21:
        S = np.flatnonzero((lens >= 12) & ok)
    S = np.sort(rng.choice(S, 21, replace=False))
    plan = _twin_plan(S, TWIN_COLS, rng)
    plan[-1] = [(c, 0) for c in EMPTY_COLS]            # reserved and never used (row -1 does not exist)
    first_code = dict((r, first) for r in behind)
    raw = _assemble(lens, K, plan, first_code, rng)
    return _finish(raw, lens, behind, S, TWIN_COLS, EMPTY_COLS, max_score)


# the longest filler row (uniform from 2) that puts 1.5 x the mean row length into (<= 16, <= 32, <= 64, <= 128, > 128)
_ROWSTATS_FILL = {1: 14, 2: 30, 4: 70, 8: 140, 16: 260}


def rowstats_matrix(G, stored_zero=False):
    """~1000 rows for k_rowstats<G>: 15 % single-entry rows, 2 % empty ones, the rest uniform in [2, hi]; every special length; the
    largest code BIG (or a stored 0) first in the row behind a row of 1, 17, 16 G + 1 and 32 G + 1 entries whose own codes are < SMALL"""
    rng = np.random.default_rng(1600 + G + (50 if stored_zero else 0))
    u = rng.random(960)
    fill = np.where(u < 0.15, 1, np.where(u < 0.17, 0, rng.integers(2, _ROWSTATS_FILL[G] + 1, 960)))
    after = sorted(set([1, 17, 16 * G + 1, 32 * G + 1]))
    lens, behind = _place(fill, special_lengths(G), rng, after)
    b = _small_matrix(lens, behind, rng, 0 if stored_zero else BIG)
    if stored_zero:                                  # (the largest code still occurs, first in the row behind the first marked one)
        s = b.raw.indptr[behind[0]]
        b.raw.data[s + 1] = BIG
    return b


def colsig_matrix(G):
    """1000 rows for k_colsig<G>: 40 % of the rows in (8 G, 16 G] entries (G > 1: more than 0.5 % of the rows are longer than 8 G),
    the rest shorter, and exactly 5 rows = 0.5 % longer than 16 G that loop up to four strides (G = 16: rows above 256 entries)"""
    rng = np.random.default_rng(1650 + G)
    cap = 16 * G
    longs = [cap + 1, 2 * cap + 1, 3 * cap + 5, 3 * cap + 16, 2 * cap]
    after = [1, 17, cap + 1, 2 * cap + 1]
    if G == 1:                                       # (the closing row of 17 entries is one of the five)
        longs, after = longs[1:], [1, 2 * cap + 1]
    specials = [x for x in special_lengths(1) if x <= cap] + longs
    n = 1000 - len(specials) - len(after) - 1
    u = rng.random(n)
    fill = np.where(u < 0.4, rng.integers(cap // 2 + 1, cap + 1, n), np.where(u < 0.55, 1, rng.integers(0, cap // 2 + 1, n)))
    lens, behind = _place(fill, specials, rng, after)
    assert len(lens) == 1000 and (lens > cap).sum() == 5
    return _small_matrix(lens, behind, rng, BIG)


WINDOW_KS = (18432, 18433, 36865)
WINDOW_COLS = (0, 18431, 18432, 18433, 36863, 36864)


def window_matrix(K):
    """300 short rows over K columns: entries in the columns at the edges of k_colsig's windows, twins across a window boundary"""
    rng = np.random.default_rng(1700 + K)
    lens = np.concatenate([rng.integers(0, 13, 260), np.full(40, 14)])
    rng.shuffle(lens)
    S = np.flatnonzero(lens == 14)[:21]
    if K == 18432:
        cols = {'pair': (0, 18431), 'score': (9000, 18430)}
    elif K == 18433:
        cols = {'pair': (18431, 18432), 'row': (0, 18430)}
    else:
        cols = {'triple': (0, 18432, 36864), 'pair': (18431, 18433), 'score': (18430, 36863), 'row': (36862, 20000)}
    plan = _twin_plan(S, cols, rng)
    plan[-1] = [(c, 0) for c in (K - 5, 17000)]
    raw = _assemble(lens, K, plan, {}, rng)
    return _finish(raw, lens, [], S, cols, (K - 5, 17000), 400)


BIG_COLUMN_ROWS = 20000


def big_column_matrix():
    """one column (5) takes 20 000 single-entry rows with scores from both ends of score_lut(65535); a second one (6) takes 300 with
    the smallest scores only; 200 short rows around them"""
    rng = np.random.default_rng(1750)
    K = 64
    n = BIG_COLUMN_ROWS + 300 + 200
    kind = rng.permutation(np.concatenate([np.zeros(BIG_COLUMN_ROWS, int), np.ones(300, int), np.full(200, 2)]))
    lens = np.where(kind == 2, rng.integers(2, 9, n), 1)
    plan = {}
    for i in np.flatnonzero(kind == 0):
        plan[int(i)] = [(5, int(rng.integers(1, 40)) if rng.random() < 0.5 else int(rng.integers(65500, 65536)))]
    for i in np.flatnonzero(kind == 1):
        plan[int(i)] = [(6, int(rng.integers(1, 4)))]
    raw = _assemble(lens, K, plan, {}, rng, hi=65000)
    raw.data[raw.indptr[np.flatnonzero(kind == 0)[0]]] = 65535
    return _finish(raw, lens, [], [], {}, (), 65535)


def wide_table_matrix():
    """the out-of-range leg: rowstats_matrix(2)'s rows on wide_table(); column 7 (empty there) takes 40 single-entry rows with the
    SMALLEST scores only — the column the old split returned as exactly 0 —, column 500 takes 30 with the largest only: the levels
    take those whole"""
    a = rowstats_matrix(2)
    uni = np.flatnonzero(np.diff(a.raw.indptr) == 1)[:70]
    indptr, indices, data = a.raw.indptr, a.raw.indices.copy(), a.raw.data.copy()
    indices[indptr[uni[:40]]] = 7
    data[indptr[uni[:40]]] = 1 + np.arange(40) % 3
    indices[indptr[uni[40:]]] = 500
    data[indptr[uni[40:]]] = 225 + np.arange(30) % 20
    b = _finish(sp.csr_matrix((data, indices, indptr), shape=a.raw.shape), np.diff(indptr), a.behind, a.S, a.cols,
                tuple(c for c in a.empty if c not in (7, 500)), 255)
    b.lut = wide_table()
    return b


MATRICES = tuple(['rowstats_%d' % g for g in LANES] + ['rowstats_zero'] + ['colsig_%d' % g for g in LANES]
                 + ['window_%d' % k for k in WINDOW_KS] + ['big_column'])
_built = {}


def matrix(name):
    """the named matrix, built once"""
    if name not in _built:
        kind, _, arg = name.partition('_')
        if name == 'rowstats_zero':
            _built[name] = rowstats_matrix(4, stored_zero=True)
        elif name == 'big_column':
            _built[name] = big_column_matrix()
        elif name == 'wide_table':
            _built[name] = wide_table_matrix()
        elif name == 'huge_table':
            _built[name] = wide_table_matrix()
            _built[name].lut = huge_table()
        else:
            _built[name] = {'rowstats': rowstats_matrix, 'colsig': colsig_matrix, 'window': window_matrix}[kind](int(arg))
    return _built[name]


def intended_lanes(name):
    """(k_rowstats lanes, k_colsig lanes) a matrix was built for; None: whatever the rule gives"""
    kind, _, arg = name.partition('_')
    if name == 'rowstats_zero':
        return 4, None
    if kind == 'rowstats':
        return int(arg), None
    if kind == 'colsig':
        return None, int(arg)
    return None, None


def shard_cut(b):
    """a row r, not a multiple of 16, that leaves the rows S[0:9] above it and S[9], S[10] below: the `row` pair of columns are twins
    inside the upper shard only"""
    r = int(b.S[9])
    if r % 16 == 0:
        r -= 1
    assert b.S[8] < r <= b.S[9] and r % 16
    return r


def shard(raw, a, z):
    return sp.csr_matrix((raw.data[raw.indptr[a]:raw.indptr[z]], raw.indices[raw.indptr[a]:raw.indptr[z]],
                          raw.indptr[a:z + 1] - raw.indptr[a]), shape=(z - a, raw.shape[1]))
