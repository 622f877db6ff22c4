"""`TelescopeLikelihood` on the MI355X engine.

Host-side mirror of the reference's operator interface
(/root/reference/telescope/utils/model.py:631-865): same constructor
(`TelescopeLikelihood(score_matrix, opts)`), same methods (`estep`, `mstep`,
`calculate_lnl`, `em`, `reassign`), same attributes (`pi`, `theta`, `pi_init`,
`theta_init`, `z`, `lnl`, `Q`, `Y`, `N`, `K`, `raw_scores`, ...), same log
lines and the same `ValueError` for a bad reassign method — so it drops in for
the scipy.sparse path behind `telescope assign` / `telescope resume`.

All arithmetic runs in libtelescope_em.so (hand-written HIP for gfx950) through
the C ABI in include/telescope_em.h.  There is no CPU fallback: constructing
the class without a usable GPU raises `EngineError`.

Multi-GPU: one process per GPU; pass `comm=` (see telescope_amd/distributed.py).
Each rank constructs the class on ITS row range of the score matrix; the global
maximum score, the setup sums and, every iteration, the per-locus column sums
are all-reduced over RCCL.
"""
import logging as lg

import numpy as np
import scipy.sparse as sp

from . import _lib
from ._lib import Engine, EngineError, Z_CUR, Z_FIRST, Z_INITIAL, Z_PREV, Z_USER  # noqa: F401

REASSIGN_METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')
_MASK_DTYPE = {'exclude': np.int8, 'choose': np.int8, 'average': np.float64,
               'conf': np.float64, 'unique': np.uint8, 'all': np.uint8}


def score_lut(max_score, scale_factor=100., mantissa_bits=53):
    """Q for every raw score 0..max_score with the reference's numpy expression
    (model.py:653 via sparse_plus.py:89-91: `raw.multiply(1./max).multiply(100.).expm1()`),
    so Q is bit-identical to the reference's.

    `mantissa_bits` < 53 rounds every Q to that many significant bits (24 = what an fp32 value format
    would store, 11 = fp16, 8 = bf16; the exponent range stays fp64's, i.e. a power-of-two scale is
    assumed): the STORAGE-precision leg of BASELINE config 3's tolerance sweep (tools/precision_sweep.py).
    The product default is 53: exact."""
    r = np.arange(int(max_score) + 1, dtype=np.uint16)
    q = np.expm1((r * (1. / max_score)) * scale_factor)
    if mantissa_bits < 53:
        m, e = np.frexp(q)
        q = np.ldexp(np.round(np.ldexp(m, mantissa_bits)), e - mantissa_bits)
    return q


EM_CHUNK = 32     # iterations enqueued per host synchronisation (Engine.em_chunk decides convergence on the device; kernels behind the converging
                  # iteration return at once: ~4 us each).  8 -> 32 in round 4: a synchronisation costs ~0.1-0.2 ms of host time, 2-3 % of a
                  # 20-iteration run of the 0.55 ms 8-GPU shard; a run that stops early pays at most 31 no-op iterations (~0.4 ms)


class _NullComm(object):
    """Single-rank stand-in for distributed.Comm."""
    rank, world = 0, 1
    in_library = True     # nothing to exchange: the engine runs whole chunks of iterations by itself

    def max_scalar(self, v):
        return v

    def sum_array(self, a):
        return a

    def max_array(self, a):
        return a

    def sum_array_u64(self, a):
        return a

    def attach(self, engine, n_cols):
        pass

    def allreduce_device(self, engine, offset=0, count=None):
        pass

    def gather_rows(self, a):
        return [a]

    def scatter_rows(self, parts):
        return parts[0]


class Assignment(object):
    """What `TelescopeLikelihood.reassign` returns: a stand-in for the reference's N x K
    `csr_matrix_plus` that answers `.sum(0)` from the device and turns into the real scipy matrix
    (rows of this rank) when anything else is asked of it."""

    def __init__(self, tl, method, thresh, which, picks):
        self._tl, self._args, self._mat, self._colsum = tl, (method, thresh, which, picks), None, None
        self.shape = (tl.N, tl.K)

    def tocsr(self):
        if self._mat is None:
            self._mat = self._tl._assignment_matrix(*self._args)
        return self._mat

    def sum(self, axis=None, **kw):
        if axis in (0, -2) and not kw and self._mat is None:
            if self._colsum is None:
                self._colsum = self._tl._colsums(*self._args)      # (picks: the tied rows only, sparse)
            return np.asarray(self._colsum).reshape(1, -1).view(np.matrix)   # scipy returns a 1 x K np.matrix: `.A1` works
        return self.tocsr().sum(axis, **kw)

    def __getitem__(self, key):
        return self.tocsr()[key]

    def __getattr__(self, name):                         # data, indices, indptr, multiply, nnz, toarray, ...
        if name.startswith('__') and name.endswith('__'):
            raise AttributeError(name)
        return getattr(self.tocsr(), name)

    def __array__(self, *a, **kw):
        return self.tocsr().toarray()


class CellFits(object):
    """What `TelescopeLikelihood.em_cells` returns: one EM fit per cell (tsem_cell_em).  Cell c touches the columns
    `cols[col_ptr[c]:col_ptr[c + 1]]` (ascending); `pi`, `theta`, `pi_init`, `theta_init` hold its parameters there, `rest[c]` the
    four values every other column of the cell has (the closed form of a column without fragments).  `n_iter`, `converged`, `lnl`
    per cell; a cell without rows is not fitted (`n_iter` 0, not converged, `lnl` NaN)."""
    FIELDS = ('col_ptr', 'cols', 'pi', 'theta', 'pi_init', 'theta_init', 'rest', 'n_iter', 'converged', 'lnl')

    def __init__(self, K, col_ptr, cols, pi, theta, pi_init, theta_init, rest, n_iter, converged, lnl):
        self.K = int(K)
        self.col_ptr, self.cols = np.asarray(col_ptr, dtype=np.int64), np.asarray(cols, dtype=np.int32)
        self.pi, self.theta = np.asarray(pi, dtype=np.float64), np.asarray(theta, dtype=np.float64)
        self.pi_init, self.theta_init = np.asarray(pi_init, dtype=np.float64), np.asarray(theta_init, dtype=np.float64)
        self.rest = np.asarray(rest, dtype=np.float64).reshape(-1, 4)
        self.n_iter = np.asarray(n_iter, dtype=np.int32)
        self.converged = np.asarray(converged).astype(bool)
        self.lnl = np.asarray(lnl, dtype=np.float64)
        self.n_cells = len(self.col_ptr) - 1
        if not (len(self.rest) == len(self.n_iter) == len(self.converged) == len(self.lnl) == self.n_cells):
            raise ValueError('CellFits: per-cell arrays of different lengths')
        n_cols = int(self.col_ptr[-1]) if self.n_cells >= 0 and len(self.col_ptr) else 0
        if any(len(a) != n_cols for a in (self.cols, self.pi, self.theta, self.pi_init, self.theta_init)):
            raise ValueError('CellFits: per-column arrays do not match col_ptr')

    def dense(self, c):
        """(pi, theta, pi_init, theta_init) of cell c as full K-vectors."""
        c = int(c)
        if not 0 <= c < self.n_cells:
            raise IndexError('cell %d outside [0, %d)' % (c, self.n_cells))
        a, b = int(self.col_ptr[c]), int(self.col_ptr[c + 1])
        out = []
        for j, src in enumerate((self.pi, self.theta, self.pi_init, self.theta_init)):
            v = np.full(self.K, self.rest[c, j])
            v[self.cols[a:b]] = src[a:b]
            out.append(v)
        return tuple(out)


BOOTSTRAP_METHODS = ('exclude', 'average', 'conf', 'unique', 'all')


def check_bootstrap_args(n_rep, method, multiplicities, n_rows):
    """The argument checks of `TelescopeLikelihood.bootstrap` (no device).  Returns the multiplicities as a C-contiguous uint8
    [n_rep x n_rows] array, or None."""
    if method == 'choose':
        raise ValueError('bootstrap: reassign mode "choose" draws from numpy\'s random stream per row and is not offered; '
                         'use one of (exclude, average, conf, unique, all)')
    if method not in BOOTSTRAP_METHODS:
        raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
    if int(n_rep) != n_rep or int(n_rep) < 1:
        raise ValueError('bootstrap: n_rep must be an integer >= 1')
    if multiplicities is None:
        return None
    m = np.asarray(multiplicities)
    if m.dtype != np.uint8:
        raise ValueError('bootstrap: multiplicities must be uint8 (0..255 copies of every row), not %s' % m.dtype)
    if m.shape != (int(n_rep), int(n_rows)):
        raise ValueError('bootstrap: multiplicities must have shape (n_rep, N) = (%d, %d), not %s' % (int(n_rep), int(n_rows), m.shape))
    return np.ascontiguousarray(m)


class BootstrapCells(object):
    """The per-cell part of a bootstrap (`BootstrapFits.cells`): statistics over the replicates of every (cell, locus) count, on the
    structural pattern of the run — the distinct (cell, locus) of the stored entries of the cells' fragments, CSR-like: cell c owns the
    slots `group_ptr[c] .. group_ptr[c + 1]`, whose loci `cols` ascend.  `mean`, `sd` (ddof 1) per slot over the `n_used` good
    replicates (those whose counts are not NaN); mean is NaN when `n_used` is 0, sd when it is below 2.  `values` [n_rep x nnz]: every
    replicate's counts (the row of a bad replicate NaN), or None when they were not kept."""

    def __init__(self, n_cells, n_cols, group_ptr, cols, mean, sd, n_used, values=None):
        self.n_cells, self.K = int(n_cells), int(n_cols)
        self.group_ptr = np.asarray(group_ptr, dtype=np.int64)
        self.cols = np.asarray(cols, dtype=np.int32)
        self.mean, self.sd = np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64)
        self.n_used = int(n_used)
        self.values = None if values is None else np.asarray(values, dtype=np.float64)
        if self.values is not None and self.values.shape[1:] != (len(self.cols),):
            raise ValueError('BootstrapCells: values must be [n_rep x slots]')
        if len(self.group_ptr) != self.n_cells + 1 or not (len(self.cols) == len(self.mean) == len(self.sd) == int(self.group_ptr[-1])):
            raise ValueError('BootstrapCells: arrays of different shapes')
        self.nnz = len(self.cols)

    def _matrix(self, data):
        m = sp.csr_matrix((np.array(data, dtype=np.float64), self.cols.copy(), self.group_ptr.copy()), shape=(self.n_cells, self.K))
        m.eliminate_zeros()                                      # (NaN is kept: it is not a zero)
        return m

    def mean_matrix(self):
        """n_cells x K scipy CSR matrix of the means, zeros dropped."""
        return self._matrix(self.mean)

    def sd_matrix(self):
        """n_cells x K scipy CSR matrix of the standard deviations, zeros dropped."""
        return self._matrix(self.sd)

    def values_matrix(self, b):
        """Replicate b's counts as an n_cells x K scipy CSR matrix, zeros dropped (needs keep_replicates=True)."""
        if self.values is None:
            raise ValueError('values_matrix: the replicates\' values were not kept (bootstrap(..., keep_replicates=True))')
        return self._matrix(self.values[b])


class BootstrapFits(object):
    """What `TelescopeLikelihood.bootstrap` returns: B refits of the model on resampled fragments.  `pi`, `theta`, `counts` are
    [B, K]; `n_frags` (the replicate's fragments, sum of its multiplicities), `n_iter`, `converged`, `lnl` per replicate; `info` =
    {'batch', 'hot_columns'}: replicates per sweep over the matrix and columns with LDS accumulators the device used.  `fitted`
    marks the replicates that were fitted (they have fragments) and have finite parameters: the statistics are taken over those."""

    def __init__(self, pi, theta, counts, n_frags, n_iter, converged, lnl, info=None, seed=0, method='exclude'):
        self.pi, self.theta = np.atleast_2d(np.asarray(pi, dtype=np.float64)), np.atleast_2d(np.asarray(theta, dtype=np.float64))
        self.counts = np.atleast_2d(np.asarray(counts, dtype=np.float64))
        self.n_frags = np.asarray(n_frags, dtype=np.int64)
        self.n_iter = np.asarray(n_iter, dtype=np.int32)
        self.converged = np.asarray(converged).astype(bool)
        self.lnl = np.asarray(lnl, dtype=np.float64)
        self.info = dict(info or {})
        self.seed, self.method = int(seed), method
        self.cells = None                                        # a BootstrapCells when the call was given `cell_of_row`
        self.n_rep = len(self.n_iter)
        if not (self.pi.shape == self.theta.shape == self.counts.shape and self.pi.shape[0] == self.n_rep ==
                len(self.n_frags) == len(self.converged) == len(self.lnl)):
            raise ValueError('BootstrapFits: arrays of different shapes')
        self.K = self.pi.shape[1]

    @property
    def fitted(self):
        return (self.n_iter > 0) & np.isfinite(self.pi).all(axis=1) & np.isfinite(self.theta).all(axis=1)

    def summary(self, level=0.95):
        """{'counts': s, 'pi': s} with s = {'mean', 'sd' (ddof 1), 'lo', 'hi'}: K-vectors over the fitted replicates; lo / hi are
        `numpy.quantile` at (1 - level) / 2 and 1 - (1 - level) / 2.  NaN where too few replicates are fitted (sd needs two)."""
        if not 0. < level < 1.:
            raise ValueError('summary: level must lie in (0, 1)')
        keep = self.fitted
        out = {}
        for name, a in (('counts', self.counts), ('pi', self.pi)):
            a = a[keep]
            nan = np.full(self.K, np.nan)
            if len(a) == 0:
                out[name] = {'mean': nan, 'sd': nan.copy(), 'lo': nan.copy(), 'hi': nan.copy()}
                continue
            lo, hi = np.quantile(a, [(1. - level) / 2., 1. - (1. - level) / 2.], axis=0)
            out[name] = {'mean': a.mean(axis=0), 'sd': a.std(axis=0, ddof=1) if len(a) > 1 else nan, 'lo': lo, 'hi': hi}
        return out


class UmiDedup(object):
    """What `umi_dedup` returns.  `rep_of_row` (int32 [N]): the representative of every row's component — the rows of one (cell, UMI)
    that are connected through shared loci (include/telescope_em.h, tsem_umi_dedup); `keep` (bool [N]): rep_of_row[i] == i, the rows a
    collapsed run keeps.  `n_class_rows`: rows with a barcode and a UMI, `n_classes`: distinct (cell, UMI) among them, `n_components`:
    molecules (components among those rows), `n_dropped`: rows that are not kept."""

    def __init__(self, rep_of_row, stats, cell_of_row):
        self.rep_of_row = np.asarray(rep_of_row, dtype=np.int32)
        self.keep = self.rep_of_row == np.arange(len(self.rep_of_row), dtype=np.int32)
        self.n_class_rows, self.n_classes, self.n_components, self.n_dropped = (int(x) for x in stats)
        self.cell_of_row = np.asarray(cell_of_row, dtype=np.int32)
        if self.cell_of_row.shape != self.rep_of_row.shape:
            raise ValueError('UmiDedup: cell_of_row must have one entry per row')

    def kept_per_cell(self, n_cells):
        """the kept rows of every cell (int64 [n_cells]; rows without barcode count nowhere)"""
        sel = self.keep & (self.cell_of_row >= 0)
        return np.bincount(self.cell_of_row[sel], minlength=int(n_cells)).astype(np.int64)


def check_umi_args(n_rows, cell_of_row, umi_of_row, n_cells=None, n_umis=None):
    """The argument checks of `umi_dedup` (no device): int32-convertible arrays with one entry per row, values from -1 on and below
    n_cells / n_umis, which are taken from the data when not given.  Returns (cell_of_row, umi_of_row, n_cells, n_umis)."""
    out = []
    for name, a, top in (('cell_of_row', cell_of_row, n_cells), ('umi_of_row', umi_of_row, n_umis)):
        a = np.asarray(a)
        if a.dtype.kind not in 'iu' or a.shape != (int(n_rows),):
            raise ValueError('umi_dedup: %s must be an integer array with one entry per row (%d), not %s %s' % (name, int(n_rows), a.dtype, a.shape))
        if a.size and (int(a.min()) < -1 or int(a.max()) >= 2 ** 31 - 1):
            raise ValueError('umi_dedup: %s must hold values from -1 (none) on that fit int32' % name)
        top = (int(a.max()) + 1 if a.size else 0) if top is None else int(top)
        if top < 0 or top > 2 ** 31 - 1 or (a.size and int(a.max()) >= top):
            raise ValueError('umi_dedup: %s holds values outside [-1, %d)' % (name, top))
        out.append((np.ascontiguousarray(a, dtype=np.int32), top))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def umi_dedup(raw_scores, cell_of_row, umi_of_row, device=0, n_cells=None, n_umis=None):
    """Collapse the UMI duplicates of a single-cell run on the device: a `UmiDedup` for the rows of `raw_scores` (the fragments x loci
    matrix of raw score codes), their cells and their UMIs (-1 = none).  Uses an engine of its own, closed afterwards; no model is
    fitted.  The collapsed run is the run on `raw_scores[d.keep]` with `cell_of_row[d.keep]`."""
    raw = raw_scores if isinstance(raw_scores, sp.csr_matrix) else sp.csr_matrix(raw_scores)
    cor, uor, n_cells, n_umis = check_umi_args(raw.shape[0], cell_of_row, umi_of_row, n_cells, n_umis)
    if raw.nnz and raw.data.dtype != np.uint16 and (raw.data.min() < 0 or raw.data.max() > 65535 or
                                                    (raw.data.dtype.kind not in 'ui' and not np.all(raw.data == np.floor(raw.data)))):
        raise ValueError('score matrix must hold integer alignment scores in [0, 65535]')
    if not raw.has_sorted_indices:                               # (the engine takes canonical CSR; the result does not depend on the order)
        raw = raw.copy()
        raw.sort_indices()
    eng = Engine(device)
    try:
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16, copy=False), raw.shape[1], None)
        rep, stats = eng.umi_dedup(cor, uor, n_cells, n_umis)
    finally:
        eng.close()
    return UmiDedup(rep, stats, cor)


class TelescopeLikelihood(object):
    """EM model over a fragments x loci score matrix (model.py:631-865)."""

    def __init__(self, score_matrix, opts, device=None, comm=None, engine=None, engine_options=None):
        """`score_matrix`, `opts` as in the reference (model.py:635-662).  Extra keywords: `device`
        (GPU index), `comm` (row-sharded runs, telescope_amd.distributed), `engine_options` — a dict for
        `tsem_set_option`, e.g. {'value_format': 1} for fp64 entries (include/telescope_em.h)."""
        self.comm = comm if comm is not None else _NullComm()
        # (a csr_matrix is taken as it is: re-wrapping one scans its index arrays, 0.8 s at 2e9 entries)
        raw = score_matrix if isinstance(score_matrix, sp.csr_matrix) else sp.csr_matrix(score_matrix)
        if engine is not None and not raw.has_canonical_format:      # (a fresh engine checks that on the device, below)
            raw = raw.copy()
            raw.sum_duplicates()
        data = raw.data
        if data.dtype != np.uint16 and raw.nnz:                      # (uint16 — what Telescope.raw_scores holds, model.py:300 — needs no check)
            if data.min() < 0 or data.max() > 65535 or \
                    (data.dtype.kind not in 'ui' and not np.all(data == np.floor(data))):
                raise ValueError('score matrix must hold integer alignment scores in [0, 65535]')
        self.raw_scores = score_matrix
        self._raw = raw
        self.N, self.K = raw.shape                                   # model.py:643
        self.scale_factor = 100.                                     # model.py:652
        engine_options = dict(engine_options or {})
        self._mantissa_bits = int(engine_options.pop('lut_mantissa_bits', 53))   # host-side knob, see score_lut
        if device is None:
            device = getattr(self.comm, 'device', 0)
        self._eng = engine if engine is not None else Engine(device)
        for key, value in engine_options.items():
            self._eng.set_option(key, int(value))
        if engine is None:
            # the matrix goes to the device first and the maximum is taken THERE (k_max_u16, 2 ms at 2e9 entries; numpy
            # needs 0.3 s, scipy's .max() 4 s); the score table follows once the global maximum is known
            try:
                self._eng.load_scores(raw.indptr, raw.indices, data.astype(np.uint16, copy=False), self.K, None)
            except EngineError as e:
                if 'canonical' not in str(e):
                    raise
                raw = raw.copy()                                     # unsorted or duplicate column ids (the device found
                raw.sum_duplicates()                                 # them): canonicalise like scipy would, load again
                if raw.nnz and raw.data.dtype != np.uint16 and raw.data.max() > 65535:
                    raise ValueError('score matrix must hold integer alignment scores in [0, 65535]')
                self._raw = raw
                self._eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16, copy=False), self.K, None)
            local_max = self._eng.max_score()
        else:
            local_max = int(data.max()) if raw.nnz else 0
        self.max_score = self.comm.max_scalar(local_max)             # model.py:640 (global)
        self._lut = score_lut(self.max_score, self.scale_factor, self._mantissa_bits) if self.max_score > 0 \
            else np.zeros(1)
        if engine is None:
            self._eng.set_lut(self._lut)

        self.epsilon = opts.em_epsilon                               # model.py:661-662
        self.max_iter = opts.max_iter
        self.pi_prior = opts.pi_prior                                # model.py:686-687
        self.theta_prior = opts.theta_prior
        if getattr(opts, 'use_likelihood', False):                   # (telescope_assign.py:439 passes it to em(): lay the matrix out for it now)
            self._eng.set_option('use_likelihood', 1)

        self._setup_model()

    @classmethod
    def from_engine(cls, engine, opts, comm=None, lut_mantissa_bits=53):
        """Wrap an engine whose score matrix is already resident (device-generated)."""
        self = cls.__new__(cls)
        self._mantissa_bits = int(lut_mantissa_bits)
        self.comm = comm if comm is not None else _NullComm()
        self.raw_scores = self._raw = None
        self._eng = engine
        self.N, self.K, _ = engine.dims()
        self.max_score = self.comm.max_scalar(engine.max_score())   # model.py:640 (global)
        self.scale_factor = 100.
        self._lut = score_lut(self.max_score, mantissa_bits=self._mantissa_bits) if self.max_score > 0 else np.zeros(1)
        engine.set_lut(self._lut)
        self.epsilon, self.max_iter = opts.em_epsilon, opts.max_iter
        self.pi_prior, self.theta_prior = opts.pi_prior, opts.theta_prior
        if getattr(opts, 'use_likelihood', False):
            engine.set_option('use_likelihood', 1)
        self._setup_model()
        return self

    def _setup_model(self):
        self.comm.attach(self._eng, self.K)
        stats, pisum0, cnt, hsh = self._eng.rowstats()               # model.py:679-699 (local)
        sums = self.comm.sum_array(np.concatenate([stats[:2], pisum0]))
        wmax = self.comm.max_array(stats[2:3])
        sig = self.comm.sum_array_u64(np.concatenate([cnt, hsh]))    # wrap-around integer sums
        cnt, hsh = sig[:self.K], sig[self.K:]
        self._total_wt, self._ambig_wt = float(sums[0]), float(sums[1])
        self._max_wt = float(wmax[0])
        self._pisum0 = np.asarray(sums[2:])
        self._pi_prior_wt = self.pi_prior * self._max_wt             # model.py:696-697
        self._theta_prior_wt = self.theta_prior * self._max_wt
        self._eng.set_model(np.array([self._total_wt, self._ambig_wt, self._max_wt]),
                            self._pisum0, cnt, hsh, self.pi_prior, self.theta_prior)
        self.pi = np.repeat(1. / self.K, self.K)                     # model.py:667
        self.theta = np.repeat(1. / self.K, self.K)                  # model.py:673
        self.pi_init = self.theta_init = None
        self.lnl = float('inf')                                      # model.py:683
        self._z = None
        self._z_which = None
        self._report_cache = {}
        self._cells_z = False                                        # the device's Z_USER buffer holds the z of em_cells
        self.n_iter, self.converged = 0, False

    # ---- lazily materialised compat attributes --------------------------------
    @property
    def Q(self):
        """model.py:653 — materialised on the host only when asked for."""
        r = self._need_raw()
        return sp.csr_matrix((self._lut[r.data], r.indices, r.indptr), shape=r.shape)

    @property
    def Y(self):
        """model.py:679 — N x 1 uint8 ambiguity indicator, as the device holds it (tsem_export_rowinfo)."""
        return self._eng.row_info()[0].reshape(-1, 1)

    @property
    def _weights(self):
        """model.py:690 — `Q.max(1)`: the N x 1 sparse column of row weights w_i, read back from the device."""
        w = self._eng.row_info()[1]
        return sp.coo_matrix(w.reshape(-1, 1))

    @property
    def z(self):
        """self.z (model.py:795): posteriors of the last E-step, on demand."""
        if self._z is None and self._z_which is not None:
            self._z = self._z_matrix(self._eng.export_z(self._z_which))
        return self._z

    @z.setter
    def z(self, value):
        """A caller-assigned z (the reference's `reassign` reads whatever `self.z` holds, model.py:837)."""
        self._z, self._z_which = value, None
        self._user_z_loaded = False
        self._report_cache = {}

    def _need_raw(self):
        if self._raw is None:
            ip, ix, rw = self._eng.export_csr()
            self._raw = sp.csr_matrix((rw, ix, ip), shape=(self.N, self.K))
        return self._raw

    def _z_matrix(self, zdata):
        """Device z (aligned to Q's pattern, -1 = not in z's pattern) -> CSR."""
        r = self._need_raw()
        keep = zdata >= 0
        if keep.all():
            return sp.csr_matrix((zdata, r.indices.copy(), r.indptr.copy()), shape=r.shape)
        rows = np.repeat(np.arange(self.N), np.diff(r.indptr))[keep]
        indptr = np.zeros(self.N + 1, dtype=r.indptr.dtype)
        np.cumsum(np.bincount(rows, minlength=self.N), out=indptr[1:])
        return sp.csr_matrix((zdata[keep], r.indices[keep], indptr), shape=r.shape)

    def _align(self, z, fill=0.0):
        """Values of sparse z laid out on Q's CSR pattern (`fill` where z has no entry)."""
        r = self._need_raw()
        z = sp.csr_matrix(z)
        if z.shape != r.shape:
            raise ValueError('z has shape %s, expected %s' % (z.shape, r.shape))
        if z.nnz == r.nnz and np.array_equal(z.indptr, r.indptr) and np.array_equal(z.indices, r.indices):
            return np.ascontiguousarray(z.data, dtype=np.float64)
        if not z.has_canonical_format:
            z = z.copy(); z.sum_duplicates()
        kq = np.repeat(np.arange(self.N, dtype=np.int64), np.diff(r.indptr)) * self.K + r.indices
        kz = np.repeat(np.arange(self.N, dtype=np.int64), np.diff(z.indptr)) * self.K + z.indices
        pos = np.searchsorted(kq, kz)
        if np.any(pos >= len(kq)) or np.any(kq[np.minimum(pos, len(kq) - 1)] != kz):
            raise ValueError('z has entries outside the score matrix pattern')
        out = np.full(r.nnz, fill, dtype=np.float64)
        out[pos] = z.data
        return out

    # ---- E / M / lnl on explicit arguments (public API) -----------------------------
    def estep(self, pi, theta):
        """model.py:702-722."""
        lg.debug('started e-step')
        return self._z_matrix(self._eng.estep(pi, theta))

    def mstep(self, z):
        """model.py:724-742."""
        lg.debug('started m-step')
        if self.comm.world > 1 and not getattr(self.comm, 'in_library', False):
            raise NotImplementedError('sharded mstep(z) needs the library communicator (nccl backend)')
        return self._eng.mstep(self._align(z))    # row-sharded: the library sums thetasum over the ranks

    def calculate_lnl(self, z, pi, theta):
        """model.py:744-760."""
        lg.debug('started lnl')
        cur = self._eng.calc_lnl(self._align(z), pi, theta)
        if self.comm.world > 1 and not getattr(self.comm, 'in_library', False):
            cur = float(self.comm.sum_array(np.array([cur]))[0])
        lg.debug('completed lnl')
        return cur

    # ---- EM loop ---------------------------------------------------------------------
    def em(self, use_likelihood=False, loglev=lg.WARNING, save_memory=True, final_lnl=True):
        """model.py:762-806 — same control flow, log lines and final state.  (`final_lnl=False`, not in the reference: skip the
        log-likelihood pass after the loop, model.py:800-801 — bench.py times the EM iterations proper with it.)

        One fused E+M device pass per iteration.  The engine runs CHUNKS of iterations without a host
        round trip (`Engine.em_chunk`): pass, all-reduce of the per-locus column sums over the library's
        RCCL communicator (row-sharded runs), update, and — decided on the device — the convergence
        test; kernels enqueued behind the converging iteration return at once, so the state after the
        call is the reference's.  The log lines of a chunk are emitted when it returns.
        """
        inum, converged, reached_max = 0, False, False
        msgD = 'Iteration {:d}, diff={:.5g}'
        msgL = 'Iteration {:d}, lnl= {:.5e}, diff={:.5g}'
        from time import perf_counter
        eng, comm, K = self._eng, self.comm, self.K
        chunked = getattr(comm, 'in_library', False)          # the engine all-reduces by itself: whole chunks per host round trip
        timeouts = 0
        timing_was = None
        if chunked and not getattr(self, 'keep_kernel_timing', False):
            timing_was = getattr(eng, 'options', {}).get('kernel_timing', 1)
            eng.set_option('kernel_timing', 0)  # per-pass HIP events are for benchmarks (Engine.kernel_stats), not for em()
        if chunked:
            eng.set_prev_lnl(self.lnl)          # model.py:786: the first lnl is compared with what the last run left (inf at first)
            if use_likelihood:
                eng.prepare_likelihood()        # the EM pass of iteration t+1 sums the lnl of iteration t (no lnl pass per iteration)
        owed = None                             # (iteration, diff) whose lnl comes with the next chunk
        while not (converged or reached_max):
            xtime = perf_counter()
            if chunked:
                want = max(1, min(EM_CHUNK, self.max_iter - inum))
                diffs, lnls, converged = eng.em_chunk(want, self.epsilon, use_likelihood, first=(inum == 0),
                                                      last=(inum + want >= self.max_iter))
                if owed is not None:
                    self.lnl = float(eng.lnl_carry)
                    lg.log(loglev, msgL.format(owed[0], self.lnl, owed[1]))
                    owed = None
                for i, diff_est in enumerate(diffs):
                    inum += 1
                    if use_likelihood:
                        if lnls[i] != lnls[i]:                 # NaN: the chunk's last iteration, summed by the next chunk's first pass
                            owed = (inum, diff_est)
                            continue
                        self.lnl = float(lnls[i])
                        lg.log(loglev, msgL.format(inum, self.lnl, diff_est))
                    else:
                        lg.log(loglev, msgD.format(inum, diff_est))
            else:
                # host-driven exchange (gloo / in-process communicators): one iteration per round trip
                eng.em_pass()                       # estep + mstep column sums (local rows)
                comm.allreduce_device(eng, 0, K + 1)   # sum over ranks; slot K carries the time-out flag
                try:
                    diff_est = eng.em_update()      # theta_hat, pi_hat, |pi_hat - pi|_1
                except EngineError as exc:          # a rank's persistent kernel timed out: nobody committed
                    timeouts += 1
                    if exc.code != _lib.ERR_TIMEOUT or timeouts > 3:
                        raise
                    eng.recover_timeout()           # that rank switches to the two-pass kernels
                    continue
                inum += 1
                if inum == 1:
                    self.pi_init, self.theta_init = eng.get_params(Z_CUR)
                if use_likelihood:
                    _lnl = self._device_lnl()
                    diff_lnl = abs(_lnl - self.lnl)
                    lg.log(loglev, msgL.format(inum, _lnl, diff_est))
                    converged = diff_lnl < self.epsilon
                    self.lnl = _lnl
                else:
                    lg.log(loglev, msgD.format(inum, diff_est))
                    converged = diff_est < self.epsilon
            reached_max = inum >= self.max_iter
            lg.debug("time: {}".format(perf_counter() - xtime))
        if timing_was is not None:
            eng.set_option('kernel_timing', timing_was)
        # A fall-back to the two-pass kernels (the persistent kernel could not keep its workgroups co-resident: a GPU shared with another
        # process, a CU mask) costs 3-6 x per iteration from then on: say so where the caller's log goes, not only on the library's stderr
        try:
            fb = int(eng.layout_info().get('fallbacks', 0))
        except Exception:                                   # noqa: BLE001 — (a tests-only engine without layout_info)
            fb = 0
        if fb > getattr(self, '_fallbacks_seen', 0):
            lg.warning('telescope_amd: the fused EM kernel fell back to the two-pass kernels (%d time(s)): this GPU is shared or masked; '
                       'iterations run 3-6x slower from here on' % fb)
            self._fallbacks_seen = fb
        if chunked:
            self.pi_init, self.theta_init = eng.get_params(Z_FIRST)
        self.pi, self.theta = eng.get_params(Z_CUR)
        self._z, self._z_which = None, Z_PREV   # z of the last E-step, exported on demand
        self._report_cache = {}
        _con = 'converged' if converged else 'terminated'
        if not use_likelihood:
            if final_lnl:
                self.lnl = eng.final_lnl() if chunked else self._device_lnl()
            else:
                self.lnl = float('nan')          # not computed (never a stale value: the next em() would seed its lnl test with it)
        self.n_iter, self.converged = inum, converged
        lg.log(loglev, 'EM {:s} after {:d} iterations.'.format(_con, inum))
        if use_likelihood or final_lnl:
            lg.log(loglev, 'Final log-likelihood: {:f}.'.format(self.lnl))
        return

    def _device_lnl(self):
        """calculate_lnl(z(prev params), cur params) without moving z (model.py:785,801)."""
        self._eng.lnl_pass()
        self.comm.allreduce_device(self._eng, self.K, 1)
        return float(self._eng.read_reduce(self.K, 1)[0])

    # ---- per-cell fits (single-cell `--pooling_mode individual`) ----------------------------------
    def _check_cells(self, cell_of_row, n_cells, what):
        if self.comm.world > 1:
            raise NotImplementedError('%s: row-sharded runs (WORLD_SIZE > 1) are not supported; run single-cell '
                                      'assignment on one GPU' % what)
        cor = np.ascontiguousarray(cell_of_row, dtype=np.int32)
        n_cells = int(n_cells)
        if cor.shape != (self.N,):
            raise ValueError('cell_of_row must have one entry per row')
        if cor.size and (cor.min() < -1 or cor.max() >= n_cells):
            raise ValueError('cell_of_row entries must lie in [-1, n_cells)')
        return cor, n_cells

    def _set_cells(self, cor, n_cells):
        """The row -> cell map on the device, once per content: the per-cell fit and the per-cell counts share it."""
        import hashlib
        key = ('cells', hashlib.blake2b(cor.tobytes(), digest_size=16).hexdigest(), n_cells)
        if getattr(self._eng, 'groups_token', None) != key:
            self._eng.set_groups(cor, n_cells)
            self._eng.groups_token = key

    def em_cells(self, cell_of_row, n_cells, use_likelihood=False, loglev=lg.WARNING):
        """One EM fit PER CELL instead of one fit of the pool: cell c's model is `TelescopeLikelihood(raw[rows of c])` with the score
        scale of the whole matrix (model.py:762-806 on the cell's rows; its own weights, totals, prior weights and pisum0; all K
        columns) — all cells in one device call (tsem_cell_em), each fitted by one workgroup, or, beyond engine option
        "cell_em_spread_entries" stored entries (a cell type), spread over the whole grid; deterministic.  The map may be any
        partition of the rows: barcodes (`--pooling_mode individual`) or cell types (`celltype`).  `cell_of_row[i]` in
        [0, n_cells) or -1 (a row in no cell), as for `reassign_cell_counts`.  Returns a `CellFits`.

        Afterwards `tl.z` is the per-cell posterior matrix (rows in no cell have no entries) and `reassign`, `reassign_colsums`,
        `reassign_cell_counts`, `reassign_group_sums` and `lookup` read it; `select_z('pooled')` switches back to the pooled fit's z
        and `select_z('cells')` to this one, without refitting.  `pi`, `theta`, `lnl`, `n_iter` stay the pooled fit's.  One GPU only."""
        cor, n_cells = self._check_cells(cell_of_row, n_cells, 'em_cells')
        self._set_cells(cor, n_cells)
        r = self._eng.cell_em(self.epsilon, self.max_iter, use_likelihood)
        fits = CellFits(self.K, *[r[k] for k in CellFits.FIELDS])
        self._pooled_which = self._z_which if self._z_which != Z_USER else getattr(self, '_pooled_which', None)
        self._cells_z = True
        self._z, self._z_which = None, Z_USER
        self._report_cache = {}
        fitted = fits.n_iter > 0
        if fitted.any():
            it = fits.n_iter[fitted]
            try:
                spread = int(self._eng.layout_info().get('cell_em_spread', 0))
            except Exception:                                   # noqa: BLE001 — (a tests-only engine without layout_info)
                spread = 0
            lg.log(loglev, 'Per-cell EM: {:d} cells fitted, {:d} converged; iterations min {:d} / median {:g} / max {:d}{}.'.format(
                int(fitted.sum()), int(fits.converged[fitted].sum()), int(it.min()), float(np.median(it)), int(it.max()),
                '; {:d} spread over the grid'.format(spread) if spread else ''))
        else:
            lg.log(loglev, 'Per-cell EM: no cell has fragments.')
        return fits

    # ---- bootstrap replicates --------------------------------------------------------------------
    def bootstrap(self, n_rep, seed=0, method='exclude', thresh=0.9, multiplicities=None, loglev=lg.WARNING, cell_of_row=None,
                  n_cells=None, keep_replicates=False):
        """`n_rep` refits of the model on RESAMPLED fragments, on the device over the resident matrix (tsem_bootstrap): replicate b
        gives row i a multiplicity m_i and is the fit of `raw[np.repeat(arange(N), m_b)]` with the score scale of the whole matrix
        (model.py:762-806; parameter stop test at `em_epsilon`, `max_iter`).  By default the m_i are Poisson(1) draws of the counter
        hash (`synthetic.bootstrap_multiplicities(seed, b, rows)`); `multiplicities`: a uint8 [n_rep x N] array instead.  Per
        replicate pi, theta, lnl and `counts` = column sums of `reassign(method, thresh)` over its fragments (`choose` is not
        offered).  Returns a `BootstrapFits`.  `tl.pi`, `tl.z`, `tl.lnl` and the per-cell fits are untouched; works before `em()`.
        One GPU only, and not with engine option "reproducible" (the replicates' column sums are unordered atomics).

        `cell_of_row` (with `n_cells`; as for `reassign_cell_counts`: [0, n_cells) or -1, a row in no cell): the same replicates,
        fitted once, also give `fits.cells`, a `BootstrapCells` — mean and sd over the replicates of every cell's count at every locus
        one of its fragments aligns to (tsem_bootstrap_groups); `keep_replicates=True` keeps every replicate's per-cell counts as
        well (n_rep x slots doubles: tests and small runs).  Without `cell_of_row`, `fits.cells` is None."""
        mult = check_bootstrap_args(n_rep, method, multiplicities, self.N)
        if self.comm.world > 1:
            raise NotImplementedError('bootstrap: row-sharded runs (WORLD_SIZE > 1) are not supported; run it on one GPU')
        if cell_of_row is None:
            if n_cells is not None or keep_replicates:
                raise ValueError('bootstrap: n_cells and keep_replicates belong to cell_of_row')
            r = self._eng.bootstrap(int(n_rep), int(seed), mult, method, thresh, self.epsilon, self.max_iter, self.K)
        else:
            if n_cells is None:
                raise ValueError('bootstrap: cell_of_row needs n_cells')
            cor, n_cells = self._check_cells(cell_of_row, n_cells, 'bootstrap')
            self._set_cells(cor, n_cells)
            r = self._eng.bootstrap_groups(int(n_rep), int(seed), mult, method, thresh, self.epsilon, self.max_iter, self.K,
                                           keep_values=keep_replicates)
        fits = BootstrapFits(r['pi'], r['theta'], r['counts'], r['n_frags'], r['n_iter'], r['converged'], r['lnl'],
                             info={'batch': int(r['info'][0]), 'hot_columns': int(r['info'][1])}, seed=seed, method=method)
        slots = ''
        if cell_of_row is not None:
            g = r['groups']
            fits.cells = BootstrapCells(n_cells, self.K, g['group_ptr'], g['cols'], g['mean'], g['sd'], g['n_used'], g['values'])
            slots = '; {:d} (cell, locus) slots'.format(fits.cells.nnz)
        keep = fits.fitted
        lg.log(loglev, 'Bootstrap: {:d} replicates, {:d} fitted, {:d} converged; iterations min {:d} / max {:d}{}.'.format(
            fits.n_rep, int(keep.sum()), int(fits.converged.sum()), int(fits.n_iter.min()), int(fits.n_iter.max()), slots))
        return fits

    def select_z(self, which):
        """Which posteriors `tl.z` and the report methods read: 'pooled' — the pooled fit's (`em()`) — or 'cells' — the per-cell
        fits' (`em_cells()`).  Nothing is refitted."""
        if which == 'cells':
            if not getattr(self, '_cells_z', False):
                raise ValueError("select_z('cells'): no per-cell posteriors on the device (em_cells(), and no z assigned since)")
            new = Z_USER
        elif which == 'pooled':
            new = getattr(self, '_pooled_which', None) if self._z_which == Z_USER else self._z_which
            if new is None:
                raise ValueError("select_z('pooled'): no pooled posteriors yet (em())")
        else:
            raise ValueError("select_z: 'pooled' or 'cells'")
        if new != self._z_which:
            self._z, self._z_which = None, new
            self._report_cache = {}

    # ---- reassign -------------------------------------------------------------------------
    def _which(self, initial):
        if initial:
            return Z_INITIAL
        if self._z_which is None:
            if self._z is None:
                raise ValueError('reassign() before em(): no posteriors yet')
            if not getattr(self, '_user_z_loaded', False):   # a caller assigned tl.z: the device reads it as is
                self._eng.set_user_z(self._align(self._z, fill=np.nan))
                self._user_z_loaded = True
                self._cells_z = False                            # (the buffer em_cells filled is replaced)
            return Z_USER
        return self._z_which

    def _report(self, which, thresh):
        """The column sums `output_report` takes from one z (model.py:432-457) — conf, exclude, average — and the rows
        with several best hits, from ONE device pass, kept until z changes (`em()`, `tl.z = ...`): the reference's
        report asks for three modes of the initial z and two of the final one, one after the other."""
        key = (which, float(thresh))
        cache = self.__dict__.setdefault('_report_cache', {})
        if key not in cache:
            other = [k for k in cache if k[0] == which]
            sums, rows, counts = self._eng.report_colsums(which, thresh)
            self._dev_ties = (which, len(rows))                  # the device keeps this pass's tie rows until the next one
            flat = self.comm.sum_array(np.concatenate([sums['conf'], sums['exclude'], sums['average']]))
            K = self.K
            rep = {'conf': flat[:K] if thresh >= 0 else None, 'exclude': np.rint(flat[K:2 * K]).astype(np.int64), 'average': flat[2 * K:],
                   'rows': rows, 'counts': counts}
            for k in other:                                        # same z, other threshold: only `conf` differs
                del cache[k]
            cache[key] = rep
        return cache[key]

    def _draw_picks(self, counts):
        """Random picks for `choose`, drawn exactly like sparse_plus.py:140-154: one draw per row with >1 best
        hits, in (global) row order, on numpy's legacy global RandomState (seeded by the caller,
        telescope_assign.py:429-431).  `counts`: this rank's tied rows' numbers of best hits, in row order."""
        parts = self.comm.gather_rows(counts)                 # rank order == global row order
        if self.comm.rank == 0:
            allc = parts[0] if len(parts) == 1 else np.concatenate(parts)
            draws = _lib.legacy_randint(allc) if allc.size else np.zeros(0, np.int32)   # == np.random.randint(0, allc), same stream
            cuts = np.cumsum([len(p) for p in parts])[:-1]
            parts = np.split(np.asarray(draws, dtype=np.int32), cuts)
        mine = self.comm.scatter_rows(parts)
        return np.zeros(0, np.int32) if mine is None else np.asarray(mine, dtype=np.int32)

    def _picks(self, which):
        """(rows, picks) of the tied rows for `choose` (sparse); consumes the caller's RNG stream NOW."""
        rep = self._report(which, self._cached_thresh(which, 0.9))   # compacted on the device: only the tied rows travel
        rows, counts = rep['rows'], rep['counts']
        return rows, self._draw_picks(counts)

    def _dense_picks(self, sparse):
        if sparse is None or len(sparse[0]) == 0:
            return None
        picks = np.zeros(self.N, dtype=np.int32)
        picks[sparse[0]] = sparse[1]
        return picks

    def reassign_colsums(self, method, thresh=0.9, initial=False):
        """`reassign(...).sum(0).A1` (model.py:435-457) without materialising the mask."""
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        which = self._which(initial)
        return self._colsums(method, thresh, which, self._picks(which) if method == 'choose' else None)

    def _colsums(self, method, thresh, which, sparse_picks):
        eng = self._eng
        if method in ('conf', 'exclude', 'average', 'choose') and which != Z_USER:
            if method == 'choose':                               # = exclude + the picked entries of the tied rows
                rep = self._report(which, self._cached_thresh(which, 0.9))
                rows, picks = sparse_picks
                on_dev = getattr(self, '_dev_ties', None) == (which, len(rows)) and rows is rep['rows']
                cs = self.comm.sum_array(eng.reassign_rows('choose', thresh, which, None if on_dev else rows, picks, n=len(rows)))
                return rep['exclude'] + np.rint(cs).astype(np.int64)
            rep = self._report(which, thresh if method == 'conf' else self._cached_thresh(which, thresh))
            return rep[method].copy()
        cs, _ = eng.reassign(method, thresh, which, self._dense_picks(sparse_picks) if method == 'choose' else None)
        cs = self.comm.sum_array(cs)
        if _MASK_DTYPE[method] != np.float64:
            cs = np.rint(cs).astype(np.int64)
        return cs

    def _cached_thresh(self, which, thresh):
        for k in self.__dict__.get('_report_cache', {}):
            if k[0] == which:
                return k[1]                                       # exclude / average do not depend on it: reuse the pass
        # No pass over this z yet, and the caller needs no `conf` column: for the INITIAL z say so (thresh < 0) — its best hits are
        # then found on the score codes alone (k_report_init_codes).  `output_report` asks exclude / choose / average of the initial z
        # and never its conf (model.py:441-446); a later reassign('conf', initial=True) runs the full pass.
        return -1.0 if which == Z_INITIAL else thresh

    def reassign_group_sums(self, method, group_rows, thresh=0.9, initial=False, group_token=None):
        """Per-group column sums of the assignment matrix: row g of the result is
        `reassign(method, thresh, initial)[group_rows[g], :].sum(0).A1` — the per-barcode count matrix
        of `scTelescope.output_report` (model.py:611-625) for `group_rows = barcode_read_indices
        .values()` — computed in one device pass, without materialising the N x K assignment.
        A row listed in several groups (or twice in one) counts once per listing, like fancy
        indexing does.  Row-sharded runs pass the indices local to this rank's rows; the sums are
        all-reduced.  The grouping's layers are cached under a hash of its CONTENT (a caller may refill the
        same list between two reports); hashing tens of millions of listings held in Python lists or sets
        costs more than the device pass, and a report asks up to six methods of one grouping — a caller that
        passes the same hashable `group_token` with the same grouping skips the hash."""
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        which = self._which(initial)
        picks = self._picks(which) if method == 'choose' else None
        layers, n_groups, digest = self._group_layers(group_rows, group_token)
        out = np.zeros((n_groups, self.K))
        for li, grp in enumerate(layers):
            # the map of a layer goes to the device once and serves every method asked of it (a report asks for up to six); the engine
            # keeps the tag of the map it holds (dropped by anyone else's set_groups): the CONTENT of the grouping, not its identity
            key = (digest, n_groups, li)
            if getattr(self._eng, 'groups_token', None) != key:
                self._eng.set_groups(grp, n_groups)
                self._eng.groups_token = key
            if li == 0:
                self._eng.reassign_groups(method, thresh, which, None, n_groups, self._dense_picks(picks), out=out)
            else:
                out += self._eng.reassign_groups(method, thresh, which, None, n_groups, self._dense_picks(picks))
        out = self.comm.sum_array(out.ravel()).reshape(out.shape)
        if _MASK_DTYPE[method] != np.float64:
            out = np.rint(out).astype(np.int64)
        return out

    def reassign_cell_counts(self, method, cell_of_row, n_cells, thresh=0.9, initial=False):
        """Per-cell count matrix of single-cell assignment (scTelescope.output_report, model.py:611-625) as a scipy CSR matrix
        (n_cells x K, float64): row c is `reassign(method, thresh, initial)[rows with cell_of_row == c, :].sum(0)`, every column added
        in ascending row order like scipy adds it — bit-identical to summing the device's own `reassign` matrix.  `cell_of_row[i]` in
        [0, n_cells) or -1 (a row in no cell).  Built sparse on the device (tsem_group_counts); `choose` draws its picks like
        `reassign('choose')`.  The map goes to the device once per content and serves every method asked of it.  One GPU only."""
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        cor, n_cells = self._check_cells(cell_of_row, n_cells, 'reassign_cell_counts')
        which = self._which(initial)
        picks = self._picks(which) if method == 'choose' else None
        self._set_cells(cor, n_cells)
        gptr, cols, vals = self._eng.group_counts(method, thresh, which, self._dense_picks(picks))
        return sp.csr_matrix((vals, cols, gptr), shape=(n_cells, self.K))

    def _group_layers(self, group_rows, token=None):
        """Row -> group maps for `reassign_group_sums`, one per LAYER: within a layer every row belongs to at most one group; the
        k-th listing of a row (over all groups, duplicates inside a group included) goes to layer k.  Built once per grouping
        (vectorised: one stable sort of the listings)."""
        import hashlib
        cached = getattr(self, '_group_layer_cache', None)
        if token is not None and cached is not None and cached[0] == ('token', token):
            return cached[1], cached[2], cached[0]              # the caller vouches for the grouping behind the token
        groups = [np.asarray(list(g) if not isinstance(g, np.ndarray) else g, dtype=np.int64) for g in group_rows]
        n_groups = len(groups)
        lens = np.array([len(g) for g in groups], dtype=np.int64)
        rows = np.concatenate(groups) if n_groups and lens.sum() else np.zeros(0, np.int64)
        # keyed on the grouping's CONTENT (a caller may refill the same list object between two reports)
        digest = ('token', token) if token is not None else \
            hashlib.blake2b(lens.tobytes() + np.ascontiguousarray(rows).tobytes(), digest_size=16).hexdigest()
        if cached is not None and cached[0] == digest:
            return cached[1], cached[2], digest
        gid = np.repeat(np.arange(n_groups, dtype=np.int32), lens)
        keep = (rows >= 0) & (rows < self.N)
        rows, gid = rows[keep], gid[keep]
        order = np.argsort(rows, kind='stable')
        rs, gs = rows[order], gid[order]
        first = np.ones(len(rs), bool)
        first[1:] = rs[1:] != rs[:-1]
        start = np.maximum.accumulate(np.where(first, np.arange(len(rs)), 0)) if len(rs) else np.zeros(0, np.int64)
        rank = np.arange(len(rs)) - start                       # 0 for a row's first listing, 1 for its second, ...
        layers = []
        for l in range(int(rank.max()) + 1 if len(rank) else 1):
            grp = np.full(self.N, -1, np.int32)
            sel = rank == l
            grp[rs[sel]] = gs[sel]
            layers.append(grp)
        self._group_layer_cache = (digest, layers, n_groups)
        return layers, n_groups, digest

    def lookup(self, ridx, fidx, method='exclude', thresh=0.9, initial=False, assignment=None):
        """`(tl.z[ridx, fidx], tl.reassign(method, thresh)[ridx, fidx])` for arrays of (fragment, locus) pairs — what
        `Telescope.update_sam` reads per alignment (model.py:483,508-511: `prob = tl.z[ridx, fidx]`, `mat[ridx, fidx] > 0`) — from
        two device passes over the DISTINCT rows asked for, without materialising either N x K matrix (`tl.z` alone is 16 GB of
        values at 2e9 stored entries).  `prob` is the z of the last E-step (0 where the pair is not in z's pattern), like `tl.z`;
        `initial` only selects the z the ASSIGNMENT is made from.  Pass `assignment=tl.reassign('choose', ...)` to look up the
        picks that object drew (a fresh `choose` draws its own, consuming the caller's RNG stream like `reassign`)."""
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        ridx = np.asarray(ridx, dtype=np.int64).ravel()
        fidx = np.asarray(fidx, dtype=np.int64).ravel()
        if ridx.shape != fidx.shape:
            raise ValueError('ridx and fidx must have the same length')
        if ridx.size and (ridx.min() < 0 or ridx.max() >= self.N or fidx.min() < 0 or fidx.max() >= self.K):
            raise IndexError('index out of range')
        which_a = self._which(initial)
        which_z = self._which(False)
        picks = None
        if method == 'choose':
            picks = assignment._args[3] if assignment is not None else self._picks(which_a)
        r = self._need_raw()
        rows, inv = np.unique(ridx, return_inverse=True)
        lens = (r.indptr[rows + 1] - r.indptr[rows]).astype(np.int64)
        off = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lens, out=off[1:])
        pk = None
        if picks is not None and len(picks[0]):                  # sparse (tied rows, picks) -> one pick per listed row
            pk = np.zeros(len(rows), np.int32)
            pos = np.searchsorted(picks[0], rows)
            hit = (pos < len(picks[0])) & (np.asarray(picks[0])[np.minimum(pos, len(picks[0]) - 1)] == rows)
            pk[hit] = np.asarray(picks[1])[pos[hit]]
        eng = self._eng
        if which_a == which_z:
            z, m = eng.rows_lookup(method, thresh, which_a, rows, off, pk)
        else:
            z, _ = eng.rows_lookup(method, thresh, which_z, rows, off, None, want_mask=False)
            _, m = eng.rows_lookup(method, thresh, which_a, rows, off, pk, want_z=False)
        # the pair's position inside its row (CSR rows are sorted): a vectorised search over the rows' slices
        key_q = inv.astype(np.int64) * self.K + fidx
        cols = np.concatenate([r.indices[r.indptr[i]:r.indptr[i + 1]] for i in rows]) if len(rows) else np.zeros(0, np.int64)
        key_e = np.repeat(np.arange(len(rows), dtype=np.int64), lens) * self.K + cols
        pos = np.searchsorted(key_e, key_q)
        found = (pos < len(key_e)) & (key_e[np.minimum(pos, max(len(key_e) - 1, 0))] == key_q) if len(key_e) else np.zeros(len(key_q), bool)
        prob = np.zeros(len(ridx))
        val = np.zeros(len(ridx))
        zf = z[pos[found]]
        prob[found] = np.where(zf < 0, 0.0, zf)                   # -1: dropped from z's pattern (an implicit zero of the CSR)
        val[found] = m[pos[found]]
        return prob, val.astype(_MASK_DTYPE[method])

    def entry_tags(self, row_begin, row_end, method='exclude', thresh=0.9, assignment=None):
        """The tag word of every stored entry of rows [row_begin, row_end), CSR order (uint32, tsem_entry_tags): bits 0-7 the MAPQ
        phred(z), 8-15 XP = int(round(z * 100)), 16 `reassign(method, thresh)[row, col] > 0`, 17 z >= 0.2 — what update_sam sets on
        a PRI alignment (model.py:503-517), with z the last E-step's (0 outside z's pattern), as `lookup` returns it.  One device
        pass, 4 B per entry.  `choose`: the picks of `assignment` (a `reassign('choose')` result) or a fresh draw, as in `lookup`.
        With option "drop_csr_indices" the column ids are rebuilt for the call and dropped again after it (`entry_tag_tiles` keeps
        them across its tiles)."""
        from .bam_out import phred_table
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        if self.comm.world > 1:
            raise NotImplementedError('entry_tags: row-sharded runs (WORLD_SIZE > 1) are not supported')
        row_begin, row_end = int(row_begin), int(row_end)
        if not 0 <= row_begin <= row_end <= self.N:
            raise IndexError('rows [%d, %d) outside [0, %d)' % (row_begin, row_end, self.N))
        which = self._which(False)
        picks = None
        if method == 'choose':
            picks = assignment._args[3] if assignment is not None else self._picks(which)
        try:
            return self._entry_tags(row_begin, row_end, method, thresh, which, picks, phred_table())
        finally:
            self._eng.entry_tags_end()                           # (ids rebuilt for this call do not stay resident: entry_tag_tiles keeps them)

    def _entry_tags(self, r0, r1, method, thresh, which, picks, tab):
        pk = None
        if picks is not None and len(picks[0]):                  # sparse (tied rows, picks) -> one pick per tile row
            rows = np.asarray(picks[0], dtype=np.int64)
            a, b = np.searchsorted(rows, r0), np.searchsorted(rows, r1)
            if b > a:
                pk = np.zeros(r1 - r0, np.int32)
                pk[rows[a:b] - r0] = np.asarray(picks[1])[a:b]
        ip = self._eng_indptr()
        return self._eng.entry_tags(method, thresh, which, r0, r1, tab, pk, n_out=int(ip[r1] - ip[r0]))

    def _eng_indptr(self):
        if self._raw is not None:
            return self._raw.indptr
        if getattr(self, '_indptr', None) is None:               # a device-generated matrix: its row pointers only (N + 1)
            self._indptr = np.empty(self.N + 1, np.int64)
            self._eng._ck(self._eng._L.tsem_export_csr(self._eng._h, self._indptr.ctypes.data, None, None))
        return self._indptr

    def entry_tag_tiles(self, method='exclude', thresh=0.9, assignment=None, tile_bytes=256 << 20):
        """Generator of (row_begin, row_end, words): `entry_tags` over the whole matrix in tiles of consecutive rows holding at most
        `tile_bytes` of words (a row longer than that is a tile of its own), so that the host never holds more than a tile.
        `choose` draws its picks once, when the generator starts, unless `assignment` carries them.  With option
        "drop_csr_indices" the device rebuilds the column ids once for all tiles and drops them again when the generator ends."""
        from .bam_out import phred_table
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        if self.comm.world > 1:
            raise NotImplementedError('entry_tags: row-sharded runs (WORLD_SIZE > 1) are not supported')
        which = self._which(False)
        picks = None
        if method == 'choose':
            picks = assignment._args[3] if assignment is not None else self._picks(which)
        tab = phred_table()
        ip = self._eng_indptr()
        cap = max(1, int(tile_bytes) // 4)
        try:
            r0 = 0
            while r0 < self.N:
                r1 = int(np.searchsorted(ip, ip[r0] + cap, side='right')) - 1
                r1 = min(self.N, max(r1, r0 + 1))
                yield r0, r1, self._entry_tags(r0, r1, method, thresh, which, picks, tab)
                r0 = r1
        finally:
            self._eng.entry_tags_end()

    def reassign(self, method, thresh=0.9, initial=False):
        """model.py:808-865 — the assignment matrix.  Returned as an `Assignment`: `.sum(0)` (all the
        reference's `output_report` asks of it, model.py:435-457) is answered by one device pass over
        the rows; anything else (`[i, j]`, `.data`, `scipy.sparse.csr_matrix(a)`, ...) builds the
        scipy CSR on first use.  `choose` draws its random picks NOW, so the caller's numpy RNG
        stream is consumed exactly where the reference consumes it."""
        if method not in REASSIGN_METHODS:
            raise ValueError('Argument "method" should be one of (exclude, choose, average, conf, unique, all)')
        which = self._which(initial)
        picks = self._picks(which) if method == 'choose' else None
        return Assignment(self, method, thresh, which, picks)

    def _assignment_matrix(self, method, thresh, which, picks):
        _, mask = self._eng.reassign(method, thresh, which, self._dense_picks(picks), want_mask=True)
        r = self._need_raw()
        keep = mask != 0
        rows = np.repeat(np.arange(self.N), np.diff(r.indptr))[keep]
        indptr = np.zeros(self.N + 1, dtype=r.indptr.dtype)
        np.cumsum(np.bincount(rows, minlength=self.N), out=indptr[1:])
        return sp.csr_matrix((mask[keep].astype(_MASK_DTYPE[method]), r.indices[keep], indptr),
                             shape=r.shape)
