"""A plain reference of what the REPORT passes add up (telescope_amd/csrc/tsem_report.hip: k_report_rows, k_report_init_codes,
k_report_pack32, k_report_slow, k_report_hist, k_group_finish — tsem_report_colsums and tsem_reassign_groups), and the seeded inputs
that tests/test_report_reference.py (CPU: this reference against the oracle) and tests/test_gpu_report_instances.py (GPU: every
kernel instance against this reference) share.  Built on tests/_rowpass_reference.py; numpy and np.longdouble only, no engine.

Expected outputs.  From the exact per-entry assignment (`exact_assigned` on the long double z): the column sums of all six methods,
the per-group sums, the rows with several best hits and their counts.  On a row that is not certain for a method (`clear` /
`clear_thresh` / `clear_pos` of _rowpass_reference: its answer hangs on the last bits of 1 / rowsum) the expected entries are the
ORACLE's, the reference implementation's own fp64 operator sequence — check 3 of tests/test_gpu_rowpass_entries.py.

Limit of a float column j, derived from the code and not tuned on any output; m_j the number of terms added into column j, e_i the
exact term:
        sum_i 2 bound(len_i) e_i  +  (m_j + 2) 2^-53 sum_i e_i
The first sum is the per-entry bound of the row pass (`average`: 1 / nb is one rounding; `conf`: z / vsum carries two z errors and
a division; k_report_pack32 adds 1.0 where the exact term is z / z = 1: inside it).  The second covers m_j atomic additions in any
order (first order: (m - 1) 2^-53 of the sum of positive terms), the flush of the LDS accumulators into the global ones and the final
n1 + n2 / 2 + shares of k_report_finish.

Inputs (`class_case`): one matrix per capacity class c of the streaming kernels, 3000 rows with lengths from {0, 1, 2, c/2, c/2 + 1,
c - 1, c}, eight rows overwritten with c + 1 (twice), 2c, 4c, 257, 513, 700 and 1025 (0.27 % of the rows: below the 0.5 % of
report_capacity), row 0 of length c, the last row of length c - 1 (its lanes read into the arrays' padding); 20 000 columns, the
rows' columns drawn from [0, span) with a log-uniform span per row, so that small column numbers are far more popular, except for
rows of 16 500 entries in all, which are dealt over as many distinct columns: more columns are in use than the LDS of k_report_rows
holds ids (about 15 200 for pi*theta, `HC`; about 10 100 accumulators for the initial z, at most 3072 for the final z, `Hs`), so
the ids of the stored entries fall on both sides of both budgets in every class (`ids_beside` counts them); scores up to 5 or up
to 400; parameters with shared pairs and planted rows (exact ties of every width in the final z, rows with an empty pattern, rows
where two entries pass conf_prob 0.45: `_parameters`).  `cold_case`: 48 000 columns, nearly all of them in use (uniform spans: more
ids than k_report_pack32's LDS table holds, or k_report_rows' in a group pass), and every row length at the
steps of its segmented scan."""
import functools

import numpy as np
import scipy.sparse as sp

import _rowpass_reference as R

LD = R.LD
U = LD(R.U)
CLASSES = (8, 16, 32, 64, 128, 256)
SCORES = (5, 400)
N_ROWS, K, K_COLD = 3000, 20000, 48000
SHARED = 0.5                # share of the columns that take (pi, theta) from the pool of four (R.parameters)
TIE_SCORES = 0.3            # share of the rows whose scores come from the two largest values (R.matrix_from_lengths)
REPORT_METHODS = ('conf', 'exclude', 'average')
GROUPS = 4
LENGTH_WEIGHTS = (0.03, 0.04, 0.05, 0.06, 0.06, 0.26, 0.50)      # of the lengths 0, 1, 2, c/2, c/2 + 1, c - 1, c (class_lengths)
COVER = 16500               # entries of a class matrix dealt over distinct columns (skewed_matrix): more than k_report_rows' LDS holds ids
SCAN_STEPS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65)     # lanes per row at which k_report_pack32's scan takes another step


def capacity_class(lens):
    """report_capacity of tsem_report.hip: the smallest class that at most 0.5 % of the rows exceed"""
    lens = np.asarray(lens)
    for c in CLASSES:
        if np.count_nonzero(lens > c) <= 0.005 * len(lens):
            return c
    return 256


def class_lengths(c, rng, n=N_ROWS):
    """(the long lengths are drawn more often: class 8 must hold more entries than the LDS of k_report_rows holds ids, `COVER`)"""
    lens = rng.choice([0, 1, 2, c // 2, c // 2 + 1, c - 1, c], n, p=LENGTH_WEIGHTS).astype(np.int64)
    over = np.array([c + 1, c + 1, 2 * c, 4 * c, 257, 513, 700, 1025])
    lens[rng.choice(np.arange(1, n - 1), len(over), replace=False)] = over
    lens[0], lens[-1] = c, c - 1
    return lens


def cold_lengths(rng, filler=5000):
    edge = sorted({l for e in (8, 16) for g in SCAN_STEPS for l in range((g - 1) * e + 1, g * e + 1)})
    lens = np.concatenate([edge, rng.randint(0, 41, filler)]).astype(np.int64)
    rng.shuffle(lens)
    return lens


def skewed_matrix(lens, k, max_score, rng, skew=True, cover=0, cap=0):
    """matrix_from_lengths' scores (and its rows of tied scores) on skewed columns: row i draws ascending columns at random gaps from
    [0, span_i), span_i log-uniform between max(len_i, 64) and k (skew False: k for every row).  cover > 0: rows of 2 .. cap entries,
    taken in random order until they hold `cover` entries, get theirs from one random permutation of the columns instead, each row
    the next len_i of it: `cover` (<= k) DISTINCT columns are then in use by rows that the streaming kernels serve themselves, however
    few entries the matrix has — the popularity ids (one per column in use, the most popular first: layout_column_map) then reach
    beyond the `cover`-th, while the skewed rows keep the small column numbers far more popular."""
    m = R.matrix_from_lengths(lens, k, max_score, rng, tie_scores=TIE_SCORES)
    lens = np.asarray(lens, dtype=np.int64)
    lo = np.maximum(lens, 64).astype(np.float64)
    span = np.floor(lo * (k / lo) ** (rng.random_sample(len(lens)) if skew else 1.0)).astype(np.int64)
    indptr = m.indptr.astype(np.int64)
    rid = R.row_ids(indptr)
    gap = (span // np.maximum(lens, 1))[rid]
    inc = np.minimum(1 + (rng.random_sample(len(rid)) * gap).astype(np.int64), gap)
    cs = np.cumsum(inc)
    start = np.concatenate([[0], cs])[indptr[:-1]]
    indices = (cs - start[rid] - 1).astype(np.int32)
    if not skew:                                                    # every other row mirrored: both ends of the range are in use
        flip = ((np.arange(len(lens)) & 1) == 1)[rid]
        back = (indptr[:-1] + indptr[1:] - 1)[rid] - np.arange(len(rid))       # the row's entries in reverse order
        indices = np.where(flip, k - 1 - indices[back], indices).astype(np.int32)
    if cover:
        perm, at = rng.permutation(k), 0
        for r in rng.permutation(np.flatnonzero((lens >= 2) & (lens <= cap))):
            if at >= cover:
                break
            indices[indptr[r]:indptr[r + 1]] = np.sort(perm[(at + np.arange(lens[r])) % k])
            at += lens[r]
        assert cover <= at <= k, (cover, at, k)
    out = sp.csr_matrix((m.data, indices, indptr), shape=(len(lens), k))
    assert out.has_sorted_indices and indices.max(initial=0) < k and np.all(np.diff(indices)[np.diff(rid) == 0] > 0)
    return out


def _parameters(raw, max_score, rng):
    """(raw with a few scores raised, pi, theta).  R.parameters' shared pairs give exact ties between numerators, but how many rows
    they tie at the TOP is left to chance (a column outside the pool usually wins a long row), so the kinds of row every leg must
    hold are planted — by construction, seen through the reference alone:
      * 70 rows of three or more entries get m of their entries (m = 2 in 25 rows, 3 .. 12 in 45) on the largest score and on
        `champion` columns, which share a pi above every other and the largest theta: two-way and wider ties at the top;
      * pi = 0 on 3 % of the other columns and on every column of 30 rows of one, two and more entries: an empty pattern;
      * 40 two-entry rows on live columns get equal scores and pi 1.1 times apart: z = 0.476 / 0.524, so both entries pass
        conf_prob 0.45 and neither lies on 0.5."""
    k = raw.shape[1]
    ip, ix, data = raw.indptr.astype(np.int64), raw.indices, raw.data.copy()
    lens = np.diff(ip)
    pi, theta = R.parameters(k, rng, shared=SHARED)
    pi_c, theta_c = pi.max(), theta.max()
    champion = np.zeros(k, bool)
    for i, r in enumerate(rng.choice(np.flatnonzero(lens >= 3), 70, replace=False)):
        m = 2 if i < 25 else rng.randint(3, min(lens[r], 12) + 1)
        pos = ip[r] + rng.choice(lens[r], m, replace=False)
        data[pos] = max_score
        champion[ix[pos]] = True
        pi[ix[pos]], theta[ix[pos]] = pi_c * (1 + 0.01 * i), theta_c       # (a pair of its own per planted row: no ties across them)
    dead = (rng.random_sample(k) < 0.03) & ~champion
    emptied = np.zeros(len(lens), bool)
    for l in sorted(set(lens[(lens > 0) & (lens <= 16)]))[:3]:
        rows = rng.choice(np.flatnonzero(lens == l), 10, replace=False)
        emptied[rows] = True
        for r in rows:
            dead[ix[ip[r]:ip[r + 1]]] = True
    pi = np.where(dead, 0.0, pi)
    two = np.flatnonzero((lens == 2) & ~emptied)
    two = two[~(dead | champion)[ix[ip[two]]] & ~(dead | champion)[ix[ip[two] + 1]]]
    for r in rng.choice(two, min(40, len(two)), replace=False):
        a, b = ip[r], ip[r] + 1
        data[b] = data[a]
        pi[ix[b]], theta[ix[b]] = 1.1 * pi[ix[a]], theta[ix[a]]
    return sp.csr_matrix((data, ix, raw.indptr), shape=raw.shape), pi, theta


@functools.lru_cache(maxsize=None)
def class_case(c, max_score):
    """(raw, lut, pi, theta) of class c, seeded"""
    from telescope_amd.likelihood import score_lut
    rng = np.random.RandomState(R._seed('report', c, max_score))
    raw, pi, theta = _parameters(skewed_matrix(class_lengths(c, rng), K, max_score, rng, cover=COVER, cap=c), max_score, rng)
    return raw, score_lut(max_score), pi, theta


@functools.lru_cache(maxsize=None)
def cold_case(max_score=400):
    from telescope_amd.likelihood import score_lut
    rng = np.random.RandomState(R._seed('report cold', max_score))
    raw, pi, theta = _parameters(skewed_matrix(cold_lengths(rng), K_COLD, max_score, rng, skew=False), max_score, rng)
    return raw, score_lut(max_score), pi, theta


def ids_beside(raw, budget, parts, hot_cols, cap):
    """(columns, entries) certainly inside and (columns, entries) certainly outside an LDS table of the `budget` lowest popularity ids,
    among the entries of rows with 2 .. cap entries (the rows a streaming kernel serves itself and that are not decided by one
    entry).  Lower bounds from the matrix and three figures of the layout, without the engine's id table (layout_column_map: columns
    go to `parts` parts in the order of their entry counts, id = slot * parts + part, a hot column takes up to 16 slots):
    the column of rank r has id < (r + 15 hot_cols + 1) parts; and the columns in use have one id each, so all but `budget` of them
    lie outside — at least the least popular ones' entries."""
    lens = np.diff(raw.indptr)
    keep = ((lens >= 2) & (lens <= cap))[R.row_ids(raw.indptr.astype(np.int64))]
    total = np.bincount(raw.indices, minlength=raw.shape[1])
    mine = np.bincount(raw.indices[keep], minlength=raw.shape[1])
    order = np.argsort(-total, kind='stable')
    n_in = max(0, min(budget // parts - 15 * hot_cols - 1, len(order)))
    inside = mine[order[:n_in]]
    used = np.sort(mine[mine > 0])
    n_out = max(0, len(used) - budget)
    return (int(np.count_nonzero(inside)), int(inside.sum())), (n_out, int(used[:n_out].sum()))


def group_map(n, seed=3):
    """row -> group: GROUPS groups and a sixth of the rows in none (-1)"""
    g = np.random.RandomState(seed).randint(-1, GROUPS + 1, n)
    return np.where(g >= GROUPS, -1, g).astype(np.int32)


class ReportReference(object):
    """Everything the checks need for one (matrix, parameters, source of z): z once (R.Reference), then per conf_prob the expected
    entries, sums, limits and tied rows."""

    def __init__(self, raw, lut, pi, theta, which):
        self.ref = R.Reference(raw, lut, pi, theta, which=which, thresh=0.9)
        self.raw, self.which = raw, which
        self.indptr, self.lens = self.ref.indptr, self.ref.lens
        self.rid = R.row_ids(self.indptr)
        self.picks = self.ref.picks
        self._entries = {}
        self._flags = {}

    def flags(self, thresh):
        """(nb exact, clear, clear_thresh, clear_pos) at this conf_prob"""
        if thresh not in self._flags:
            r = self.ref
            self._flags[thresh] = R.exact_assigned(self.indptr, r.z, r.inpat, thresh, methods=())[1:]
        return self._flags[thresh]

    def certain_rows(self, method, thresh):
        nb, clear, clear_thresh, clear_pos = self.flags(thresh)
        return R.clear_rows(method, clear, clear_thresh, clear_pos)

    def unclear_rows(self, thresh):
        """(rows whose `exclude` / `average` or `conf` entries are the oracle's, those among them that are there only because their
        largest z is 1 to rounding while conf_prob is 1: z cannot exceed 1, so such a row sits ON that threshold whatever the inputs —
        every row of one entry does)"""
        r = self.ref
        unclear = ~(self.certain_rows('exclude', thresh) & self.certain_rows('conf', thresh))
        zmax = R._row_reduce(np.maximum, np.where(r.inpat, r.z, LD(-1)), self.indptr, LD(-1))
        on_one = unclear & self.certain_rows('exclude', thresh) & (thresh >= 1.0) & (zmax >= 1 - 2 * R.bound(self.lens))
        return unclear, on_one

    def entries(self, method, thresh):
        """the expected value per stored entry, long double: exact on certain rows, the oracle's elsewhere"""
        key = (method, thresh)
        if key not in self._entries:
            r = self.ref
            e = R.exact_assigned(self.indptr, r.z, r.inpat, thresh, self.picks, methods=(method,))[0][method].astype(LD)
            c = self.certain_rows(method, thresh)
            if not c.all():
                o = R.oracle_assigned(r.om, self.raw, method, thresh, self.which, self.picks).astype(LD)
                e = np.where(c[self.rid], e, o)
            self._entries[key] = e
        return self._entries[key]

    def best_counts(self, thresh):
        nb, clear = self.flags(thresh)[:2]
        return np.where(clear, nb, self.ref.nbo)

    def ties(self, thresh):
        nb = self.best_counts(thresh)
        rows = np.flatnonzero(nb > 1)
        return rows.astype(np.int32), nb[rows].astype(np.int32)

    def sums(self, method, thresh, keep_rows=None):
        """(expected [K], limit [K]) in long double; keep_rows: a mask of the rows that count"""
        e = self.entries(method, thresh)
        k = self.raw.shape[1]
        if keep_rows is not None:
            e = np.where(keep_rows[self.rid], e, LD(0))
        cols = self.raw.indices
        s, b, m = np.zeros(k, LD), np.zeros(k, LD), np.zeros(k, np.int64)
        np.add.at(s, cols, e)
        np.add.at(b, cols, 2 * R.bound(self.lens)[self.rid] * e)
        np.add.at(m, cols, (e != 0).astype(np.int64))
        return s, b + (m + 2).astype(LD) * U * s

    def group_sums(self, method, thresh, group, n_groups):
        out = [self.sums(method, thresh, group == g) for g in range(n_groups)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def census(self, thresh):
        """rows by kind, from the reference alone"""
        r = self.ref
        nb = self.flags(thresh)[0]
        unclear, on_one = self.unclear_rows(thresh)
        zmax = R._row_reduce(np.maximum, np.where(r.inpat, r.z, LD(-1)), self.indptr, LD(-1))
        passing = np.bincount(self.rid[r.inpat & (r.z >= LD(thresh))], minlength=len(self.lens))
        return dict(single=int((nb == 1).sum()), two_way=int((nb == 2).sum()), wider=int((nb > 2).sum()),
                    empty=int((nb == 0).sum()), conf=int((passing > 0).sum()), conf_several=int((passing > 1).sum()),
                    unclear=int((unclear & ~on_one).sum()), on_one=int(on_one.sum()),
                    near_one=int((zmax >= 1 - 2 * R.bound(self.lens)).sum()))


@functools.lru_cache(maxsize=None)
def reference(c, max_score, which):
    """the shared ReportReference of a class matrix (c = 'cold': the COLD matrix)"""
    raw, lut, pi, theta = cold_case(max_score) if c == 'cold' else class_case(c, max_score)
    return ReportReference(raw, lut, pi, theta, which)


def fraction(got, want, limit):
    """the largest |got - want| / limit over the columns; a column whose limit is 0 must be exact (inf otherwise)"""
    err = np.abs(np.asarray(got).astype(LD) - want)
    frac = np.zeros(err.shape, LD)
    pos = limit > 0
    frac[pos] = err[pos] / limit[pos]
    frac[~pos & (err > 0)] = np.inf
    return float(frac.max()) if frac.size else 0.0
