"""Reference for the per-cell EM fits (`TelescopeLikelihood.em_cells`): the oracle, run once per cell on the cell's rows with the
score scale of the whole matrix, and what the tests derive from its results.  Shared by tests/test_gpu_cell_em.py,
tests/test_gpu_cell_em_edges.py and tests/test_cell_em_host.py; every reference is computed once per shape and never changed."""
import functools
import warnings

import numpy as np
import scipy.sparse as sp

RTOL = 1e-9
ALL_METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')
INT_METHODS = ('exclude', 'choose', 'unique', 'all')

# seed: (rows, K, cells, theta_prior, pi_prior, use_likelihood).  1-5: the issue's shapes; 6: cells whose tables take the largest LDS
# class (1024 < Kc <= 3840), which none of the first five reaches.
SHAPES = {
    1: (6000, 300, 40, 200000, 0, False),
    2: (6000, 2000, 200, 200000, 0, False),
    3: (5000, 60, 25, 0, 0, False),
    4: (5000, 500, 30, 5, 1, True),
    5: (20000, 6000, 3, 200000, 0, False),
    6: (9000, 2500, 4, 200000, 0, False),
}
EPSILON, MAX_ITER = 1e-7, 100


def random_matrix(seed, n, k, n_cells):
    """Row lengths 1-11, 30 % of the rows forced to one entry, scores 100-399; cells drawn uniformly, 10 % of the rows in no cell."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, min(k, 12), n)
    lens[rng.rand(n) < 0.3] = 1
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    raw = sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), indices, indptr), shape=(n, k))
    cor = rng.randint(0, n_cells, n).astype(np.int32)
    cor[rng.rand(n) < 0.1] = -1
    return raw, cor


class CellRef(object):
    """The oracle's fit of every cell: `fits[c]` is the cell's OracleModel (None for a cell without rows), `rows[c]` its rows."""

    def __init__(self, raw, cor, n_cells, pi_prior, theta_prior, epsilon=EPSILON, max_iter=MAX_ITER, use_likelihood=False):
        from oracle.telescope_oracle import OracleModel
        self.raw, self.cor, self.n_cells = sp.csr_matrix(raw), np.asarray(cor), int(n_cells)
        self.N, self.K = self.raw.shape
        gmax = self.raw.max()
        self.rows = [np.flatnonzero(self.cor == c) for c in range(self.n_cells)]
        self.fits = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                   # (theta = NaN at theta_prior = 0 divides 0 by 0, as the closed form says)
            for rows in self.rows:
                if len(rows) == 0:
                    self.fits.append(None)
                    continue
                om = OracleModel(self.raw[rows], pi_prior, theta_prior, max_score=gmax)
                om.trace = om.em(epsilon, max_iter, use_likelihood)    # [(diff, lnl or None)] per iteration
                self.fits.append(om)

    @functools.lru_cache(maxsize=None)
    def z(self):
        """The cells' z assembled into one N x K matrix (rows in no cell are empty)."""
        r, c, v = [], [], []
        for rows, om in zip(self.rows, self.fits):
            if om is None:
                continue
            zc = sp.coo_matrix(om.z)
            r.append(rows[zc.row]); c.append(zc.col); v.append(zc.data)
        if not r:
            return sp.csr_matrix((self.N, self.K))
        m = sp.csr_matrix((np.concatenate(v), (np.concatenate(r), np.concatenate(c))), shape=(self.N, self.K))
        m.sort_indices()
        return m

    def pooled_model(self, pi_prior=0, theta_prior=200000):
        """A pooled OracleModel whose `.z` is the cells' z: its `reassign` is the per-cell assignment matrix."""
        from oracle.telescope_oracle import OracleModel
        om = OracleModel(self.raw, pi_prior, theta_prior)
        om.z = self.z()
        return om

    def twin_classes(self, c):
        """Columns of cell c with the same rows and the same scores, as lists of column ids (classes of two or more)."""
        sub = sp.csc_matrix(self.raw[self.rows[c]])
        seen = {}
        for j in np.flatnonzero(np.diff(sub.indptr)):
            a, b = sub.indptr[j], sub.indptr[j + 1]
            seen.setdefault((sub.indices[a:b].tobytes(), sub.data[a:b].tobytes()), []).append(int(j))
        return [cols for cols in seen.values() if len(cols) > 1]

    @functools.lru_cache(maxsize=None)
    def undecided_rows(self, conf_prob=0.9):
        """Rows the oracle cannot decide, judged by its own z: the two largest values of the row differ by less than 1e-9 relative
        without being equal; or they are equal on columns that are not twins in the row's cell; or a value lies within 1e-9 of
        conf_prob."""
        out = []
        for c, (rows, om) in enumerate(zip(self.rows, self.fits)):
            if om is None:
                continue
            z = sp.csr_matrix(om.z)
            twin_of = {}
            for t, cols in enumerate(self.twin_classes(c)):
                for j in cols:
                    twin_of[j] = t
            for i in range(z.shape[0]):
                a, b = z.indptr[i], z.indptr[i + 1]
                v, cols = z.data[a:b], z.indices[a:b]
                if len(v) == 0 or np.any(np.isnan(v)):
                    continue
                if np.any(np.abs(v - conf_prob) <= RTOL * conf_prob):
                    out.append(rows[i]); continue
                if len(v) < 2:
                    continue
                order = np.argsort(v)
                top, second = v[order[-1]], v[order[-2]]
                if top != second:
                    if top - second < RTOL * top:
                        out.append(rows[i])
                    continue
                best = cols[v == top]
                classes = {twin_of.get(int(j), -1 - int(j)) for j in best}
                if len(classes) > 1:
                    out.append(rows[i])
        return np.asarray(sorted(out), dtype=np.int64)

    def fitted_rows(self):
        return int(sum(len(r) for r, om in zip(self.rows, self.fits) if om is not None))


@functools.lru_cache(maxsize=None)
def shape_case(seed):
    n, k, n_cells, theta_prior, pi_prior, use_lnl = SHAPES[seed]
    raw, cor = random_matrix(seed, n, k, n_cells)
    return raw, cor, n_cells, CellRef(raw, cor, n_cells, pi_prior, theta_prior, use_likelihood=use_lnl)


def boundary_matrix(seed, K, cells):
    """A matrix whose cells have exactly the compacted column count and the entry count asked for: `cells` = [(Kc, entries), ...]
    with Kc <= entries.  Per cell: Kc distinct columns of K; the entries laid cyclically over them; cut into rows of 1-8 entries
    (30 % of the rows forced to one entry, lengths capped by Kc, so a row never meets a column twice); indices sorted per row, scores
    100-399; the rows of all cells shuffled together.  Returns (raw, cell_of_row, [sorted columns of every cell])."""
    rng = np.random.RandomState(seed)
    lens, idx, cell, cols_of = [], [], [], []
    for c, (kc, ne) in enumerate(cells):
        assert 1 <= kc <= K and ne >= kc, (c, kc, ne)
        cols = rng.choice(K, kc, replace=False)
        seq = cols[np.arange(ne) % kc]
        o = 0
        while o < ne:
            l = 1 if rng.rand() < 0.3 else int(rng.randint(1, 9))
            l = min(l, kc, ne - o)
            idx.append(np.sort(seq[o:o + l])); lens.append(l); cell.append(c)
            o += l
        cols_of.append(np.sort(cols).astype(np.int32))
    perm = rng.permutation(len(lens))
    indptr = np.concatenate([[0], np.cumsum(np.asarray(lens)[perm])])
    indices = np.concatenate([idx[i] for i in perm]).astype(np.int32)
    raw = sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), indices, indptr), shape=(len(lens), K))
    return raw, np.asarray(cell, np.int32)[perm], cols_of


# Boundary case B: a cell on either side of every class threshold of the device unit (Kc 256 / 1024 / 3840 columns, 4096 entries
# for the wave class), the largest LDS launch the unit can make (Kc = 3840), and three tiny cells.  Classes: wave 4 (cells 0, 7, 8,
# 9), 256 threads 3 (1, 2, 3), 512 threads 2 (4, 5), global workspace 1 (6).  Seed 21, checked on the CPU
# (tests/test_cell_em_host.py::test_boundary_case_is_decided_by_no_rounding): every cell is fitted without a NaN, in 2-100
# iterations (four cells run into max_iter under the first parameter set), 5 and 22 of 10016 rows are undecided, and no
# iteration's stop test lies within 1e-6 relative of epsilon — so no other seed was needed.
B_SEED, B_K = 21, 4000
B_CELLS = ((256, 4096), (257, 4096), (256, 4097), (1024, 3000), (1025, 3000), (3840, 8000), (3841, 8000), (1, 1), (1, 40), (2, 2))
B_CLASSES = (4, 3, 2, 1)
B_PARAMS = ((0, 200000, False), (1, 5, True))              # (pi_prior, theta_prior, use_likelihood)


@functools.lru_cache(maxsize=None)
def boundary_case():
    return boundary_matrix(B_SEED, B_K, B_CELLS)


def _boundary_named():
    raw, cor, _ = boundary_case()
    return raw, cor, len(B_CELLS)


# the two cells around the largest LDS launch alone (engine options are tested on them)
LARGE_CELLS = ((3840, 8000), (3841, 8000))


@functools.lru_cache(maxsize=None)
def large_case():
    raw, cor, _ = boundary_matrix(22, B_K, LARGE_CELLS)
    return raw, cor, len(LARGE_CELLS)


def empty_rows(raw, rows):
    """`raw` with the stored entries of `rows` removed (the rows stay)."""
    raw = sp.csr_matrix(raw)
    lens = np.diff(raw.indptr)
    keep = np.ones(raw.shape[0], bool)
    keep[rows] = False
    ek = np.repeat(keep, lens)
    indptr = np.concatenate([[0], np.cumsum(lens * keep)])
    return sp.csr_matrix((raw.data[ek], raw.indices[ek], indptr), shape=raw.shape)


@functools.lru_cache(maxsize=None)
def empty_rows_case():
    """300 x 40, six random cells; five rows lose their entries: three stay in their (otherwise normal) cells, the other two
    become cell 6, a cell of rows without entries only (Kc = 0)."""
    raw, cor = random_matrix(7, 300, 40, 6)
    rows = np.flatnonzero(cor >= 0)[[0, 10, 20, 30, 40]]
    raw = empty_rows(raw, rows)
    cor = cor.copy()
    cor[rows[3:]] = 6
    return raw, cor, 7


@functools.lru_cache(maxsize=None)
def full_columns_case():
    """cell 0 touches every column (Kc == K: no `rest` column exists)"""
    raw, cor, _ = boundary_matrix(3, 64, [(64, 500), (3, 7)])
    return raw, cor, 2


@functools.lru_cache(maxsize=None)
def tiny_k_case(K):
    raw, cor, _ = boundary_matrix(5, K, {2: [(2, 30), (1, 4)], 1: [(1, 5), (1, 1)]}[K])
    return raw, cor, 2


NAMED = {'B': _boundary_named, 'large': large_case, 'empty_rows': empty_rows_case, 'full_columns': full_columns_case,
         'K2': functools.partial(tiny_k_case, 2), 'K1': functools.partial(tiny_k_case, 1),
         'shape1': lambda: shape_case(1)[:3]}


@functools.lru_cache(maxsize=None)
def cell_ref(key,pi_prior, theta_prior, use_likelihood=False, max_iter=MAX_ITER):
    """The oracle's fits of a named matrix (NAMED), once per session."""
    raw, cor, n_cells = NAMED[key]()
    return CellRef(raw, cor, n_cells, pi_prior, theta_prior, max_iter=max_iter, use_likelihood=use_likelihood)


def stop_margin(ref, epsilon=EPSILON):
    """The smallest relative distance |x - epsilon| / epsilon of any iteration's stop test x (diff, or the step of lnl) of any cell:
    iteration counts are compared for equality and must not hinge on a rounding."""
    worst = np.inf
    for om in ref.fits:
        if om is None:
            continue
        lnl_prev = np.inf
        for diff, lnl in om.trace:
            x = diff if lnl is None else abs(lnl - lnl_prev)
            if lnl is not None:
                lnl_prev = lnl
            if np.isfinite(x):
                worst = min(worst, abs(x - epsilon) / epsilon)
    return worst


def _check_fits(fits, ref, label):
    """n_iter / converged equal; pi, theta, pi_init, theta_init (full K) and lnl at RTOL; a cell without rows is not fitted."""
    assert fits.n_cells == ref.n_cells
    for c, om in enumerate(ref.fits):
        if om is None:
            assert fits.n_iter[c] == 0 and not fits.converged[c] and np.isnan(fits.lnl[c]), (label, c)
            assert fits.col_ptr[c + 1] == fits.col_ptr[c]
            continue
        assert fits.n_iter[c] == om.n_iter and bool(fits.converged[c]) == bool(om.converged), \
            (label, c, int(fits.n_iter[c]), om.n_iter, bool(fits.converged[c]), om.converged)
        cols = fits.cols[fits.col_ptr[c]:fits.col_ptr[c + 1]]
        assert np.array_equal(cols, np.unique(ref.raw[ref.rows[c]].indices)), (label, c)
        for got, want, name in zip(fits.dense(c), (om.pi, om.theta, om.pi_init, om.theta_init), ('pi', 'theta', 'pi_init', 'theta_init')):
            assert np.allclose(got, want, rtol=RTOL, atol=0, equal_nan=True), (label, c, name, np.nanmax(np.abs(got - want)))
        assert np.isclose(fits.lnl[c], om.lnl, rtol=RTOL, atol=0, equal_nan=True), (label, c, fits.lnl[c], om.lnl)


def _check_z(tl, ref, label):
    """Same pattern, stored entries at RTOL; rows in no cell have no entries.  A cell whose oracle z is NaN (theta = NaN spreads
    through 0 * NaN, model.py:718-720) has no entries on the device: NaN is the device's mark for `not in z's pattern`."""
    got = sp.csr_matrix(tl.z); got.sort_indices()
    want = ref.z()
    nan_rows = np.zeros(ref.N, bool)
    if want.nnz:
        nan_rows[np.unique(sp.coo_matrix(want).row[np.isnan(want.data)])] = True
    glen, wlen = np.diff(got.indptr), np.diff(want.indptr)
    assert np.all(glen[ref.cor < 0] == 0), label
    assert np.all(glen[nan_rows] == 0), label
    keep = ~nan_rows
    assert np.array_equal(glen[keep], wlen[keep]), label
    w = want[np.flatnonzero(keep)]
    g = got[np.flatnonzero(keep)]
    assert np.array_equal(g.indices, w.indices), label
    assert np.allclose(g.data, w.data, rtol=RTOL, atol=0), (label, np.max(np.abs(g.data - w.data)))


def selector(cor, n_cells):
    """n_cells x N 0/1 matrix: S @ A adds every column in ascending row order from 0, like A[rows].sum(0)."""
    cor = np.asarray(cor)
    keep = np.flatnonzero(cor >= 0)
    return sp.csr_matrix((np.ones(len(keep)), (cor[keep], keep)), shape=(n_cells, len(cor)))


def twin_tie_matrix(seed=17, n=400, n_cells=20):
    """A matrix whose ties are all twin ties: every ambiguous row sits, with one score, on a pair of columns that no other row
    touches; unique rows share 50 further columns.  Both sides of a comparison then draw `choose` for the same rows."""
    rng = np.random.RandomState(seed)
    amb = rng.rand(n) < 0.7
    k = 2 * n + 50
    r, c, v = [], [], []
    for i in range(n):
        s = int(rng.randint(100, 400))
        if amb[i]:
            r += [i, i]; c += [2 * i, 2 * i + 1]; v += [s, s]
        else:
            r.append(i); c.append(2 * n + int(rng.randint(50))); v.append(s)
    raw = sp.csr_matrix((np.asarray(v, dtype=np.uint16), (r, c)), shape=(n, k))
    raw.sort_indices()
    cor = rng.randint(0, n_cells, n).astype(np.int32)
    return raw, cor, n_cells


def emulate_cell(raw_c, lut, k_total, pi_prior, theta_prior, epsilon, max_iter, use_likelihood):
    """The device unit's arithmetic for one cell, in numpy, on the cell's compacted columns: state for the Kc columns the cell
    touches, one closed-form value for the K - Kc others (they count in diff).  Returns (cols, pi, theta, rest_pi, rest_theta,
    n_iter, converged, lnl).  Keeps the host tests honest about the closed form without a device."""
    raw_c = sp.csr_matrix(raw_c)
    cols = np.unique(raw_c.indices)
    q = sp.csr_matrix((lut[raw_c.data], np.searchsorted(cols, raw_c.indices), raw_c.indptr), shape=(raw_c.shape[0], len(cols)))
    lens = np.diff(q.indptr)
    y = (lens > 1).astype(float)
    w = np.asarray(q.max(1).todense()).ravel() if q.nnz else np.zeros(q.shape[0])
    tw, aw, wm = w.sum(), (w * y).sum(), (w.max() if len(w) else 0.0)
    ppw, tpw = pi_prior * wm, theta_prior * wm
    rid = np.repeat(np.arange(q.shape[0]), lens)
    ps0 = np.bincount(q.indices, weights=q.data * (1 - y[rid]), minlength=len(cols))
    kc = len(cols)
    pi = np.full(kc, 1. / k_total); th = pi.copy()
    rp = rt = 1. / k_total
    it, conv, lnl_prev = 0, False, np.inf

    def numer(p, t):
        return (q.data * y[rid]) * (p * t)[q.indices] + (q.data * (1 - y[rid])) * p[q.indices]

    def lnl_of(pp, tp, p, t):
        n = numer(pp, tp)
        rs = np.bincount(rid, weights=n, minlength=q.shape[0])
        z = n * np.where(rs > 0, 1. / np.where(rs > 0, rs, 1), 0.)[rid]
        m = numer(p, t)
        keep = (n != 0) & (m != 0)
        return float((z[keep] * np.log1p(m[keep])).sum())
    while True:
        pp, tp, rpp = pi, th, rp
        n = numer(pp, tp)
        rs = np.bincount(rid, weights=n, minlength=q.shape[0])
        z = n * np.where(rs > 0, 1. / np.where(rs > 0, rs, 1), 0.)[rid]
        s = np.bincount(q.indices, weights=np.where(n != 0, (z * w[rid]) * y[rid], 0.), minlength=kc)
        th = (s + tpw) / (aw + tpw * k_total)
        pi = ((ps0 + s) + ppw) / (tw + ppw * k_total)
        rt = tpw / (aw + tpw * k_total)
        rp = ppw / (tw + ppw * k_total)
        it += 1
        diff = np.abs(pi - pp).sum() + (k_total - kc) * abs(rp - rpp)
        if use_likelihood:
            lnl = lnl_of(pp, tp, pi, th)
            conv = abs(lnl - lnl_prev) < epsilon
            lnl_prev = lnl
        else:
            conv = diff < epsilon
        if conv or it >= max_iter:
            break
    return cols, pi, th, rp, rt, it, conv, lnl_of(pp, tp, pi, th)
