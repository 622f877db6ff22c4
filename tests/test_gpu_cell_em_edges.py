"""Per-cell EM fits on the device (tsem_cell_em, `tl.em_cells`) where the random shapes of tests/test_gpu_cell_em.py do not go: a cell
on either side of every threshold between the unit's four kernels (and the largest LDS launch it can make), `use_likelihood` and a
pi prior in every class, a cell's fit as a function of the cell alone, repeated calls on one handle and its cached layout, the
engine's layout options, and degenerate cells — rows without entries, Kc = 0, Kc = K, K of 1 and 2, one iteration, no pooled fit.

The reference is always the oracle run per cell (tests/_cell_em_reference.py, RTOL = 1e-9, atol 0), computed once per session; what
is stated as identical is compared as bits.  profiles/r12_cell_em_tests.txt keeps a run with the time of every test."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
import _cell_em_reference as R
from _cell_em_reference import _check_fits, _check_z

pytestmark = pytest.mark.gpu
COLUMN_ARRAYS = ('cols', 'pi', 'theta', 'pi_init', 'theta_init')
CELL_ARRAYS = ('rest', 'n_iter', 'converged', 'lnl')
CLASS_NAMES = ('cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global')
PRIORS = ((0, 200000), (1, 5), (0, 0))                     # (pi_prior, theta_prior) of the degenerate cases
OPTION_SETS = [{'value_format': 1}, {'value_format': 2}, {'split': 1, 'parts': 6}, {'drop_csr_indices': 1}, {'reproducible': 1},
               {'hot_split': 0}]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _tl(raw, pi_prior=0, theta_prior=200000, options=None, pooled_iters=5):
    """A fresh object with a pooled fit (a few iterations: it only has to exist, and it lays the matrix out as `options` ask)."""
    from telescope_amd.likelihood import TelescopeLikelihood
    tl = TelescopeLikelihood(raw, Opts(pi_prior=pi_prior, theta_prior=theta_prior, max_iter=pooled_iters), engine_options=options)
    tl.em()
    tl.max_iter = R.MAX_ITER
    return tl


def _z_aligned(tl):
    """The per-cell z as the device exports it: one value per stored entry of the matrix, -1 outside z's pattern."""
    from telescope_amd import _lib
    return tl._eng.export_z(_lib.Z_USER)


def _classes(eng):
    info = eng.layout_info()
    return tuple(info[n] for n in CLASS_NAMES)


def _cell(fits, c):
    """Everything the fit says about cell c."""
    a, b = int(fits.col_ptr[c]), int(fits.col_ptr[c + 1])
    out = {name: getattr(fits, name)[a:b] for name in COLUMN_ARRAYS}
    out.update({name: getattr(fits, name)[c] for name in CELL_ARRAYS})
    return out


def _assert_same_cell(got, want, label):
    for name in COLUMN_ARRAYS + CELL_ARRAYS:
        assert _same_bits(got[name], want[name]), (label, name, got[name], want[name])


def _assert_same_fit(a, za, b, zb, label):
    """two fits of the same map: every array and the aligned z, bit for bit"""
    from telescope_amd.likelihood import CellFits
    for name in CellFits.FIELDS:
        assert _same_bits(getattr(a, name), getattr(b, name)), (label, name)
    assert _same_bits(za, zb), (label, 'z')


def _entries_of(raw, rows):
    """positions of the stored entries of `rows` in the matrix's CSR order"""
    return np.flatnonzero(np.isin(np.repeat(np.arange(raw.shape[0]), np.diff(raw.indptr)), rows))


class _EngineFit(object):
    """The engine-level path, no TelescopeLikelihood and no pooled fit: load_scores -> rowstats -> set_model -> set_groups -> cell_em;
    `.z` from the Z_USER export."""

    def __init__(self, device, raw, cor, n_cells, pi_prior, theta_prior, use_likelihood=False):
        from telescope_amd import _lib
        from telescope_amd.likelihood import CellFits, score_lut
        raw = sp.csr_matrix(raw)
        self.eng = eng = _lib.Engine(device)
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], score_lut(int(raw.max())))
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, pi_prior, theta_prior)
        eng.set_groups(cor, n_cells)
        r = eng.cell_em(R.EPSILON, R.MAX_ITER, use_likelihood)
        self.fits = CellFits(raw.shape[1], *[r[k] for k in CellFits.FIELDS])
        self.z_aligned = eng.export_z(_lib.Z_USER)
        keep = self.z_aligned >= 0                           # (-1: not in z's pattern)
        rid = np.repeat(np.arange(raw.shape[0]), np.diff(raw.indptr))
        self.z = sp.csr_matrix((self.z_aligned[keep], (rid[keep], raw.indices[keep])), shape=raw.shape)


# ---- a. the class boundaries ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary_fit(params):
    pi_prior, theta_prior, use_lnl = params
    raw, cor, _ = R.boundary_case()
    tl = _tl(raw, pi_prior, theta_prior)
    fits = tl.em_cells(cor, len(R.B_CELLS), use_likelihood=use_lnl)
    return tl, fits, _z_aligned(tl), _classes(tl._eng)


@pytest.mark.parametrize('params', R.B_PARAMS)
def test_cells_on_both_sides_of_every_class_boundary(gpu_device, params):
    """Case B (tests/_cell_em_reference.py): Kc 256 | 257, 4096 | 4097 entries, 1024 | 1025, 3840 | 3841 and three tiny cells, by the
    sum of |pi - previous pi| and by the likelihood with a pi prior: the oracle's fits and z, the class every cell went to, and the
    columns every cell was drawn with."""
    tl, fits, _, classes = _boundary_fit(params)
    raw, cor, cols = R.boundary_case()
    ref = R.cell_ref('B', *params)
    assert raw.shape[1] == R.B_K and [len(c) for c in cols] == [kc for kc, _ in R.B_CELLS]
    assert [raw[cor == c].nnz for c in range(len(R.B_CELLS))] == [ne for _, ne in R.B_CELLS]
    print('case B %s: iterations %s, classes %s' % (params, fits.n_iter.tolist(), classes))
    assert classes == R.B_CLASSES, classes
    for c, want in enumerate(cols):
        assert np.array_equal(fits.cols[fits.col_ptr[c]:fits.col_ptr[c + 1]], want), c
    _check_fits(fits, ref, ('B', params))
    _check_z(tl, ref, ('B', params))


# ---- b. a cell's fit does not depend on its companions ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary_scratch(params):
    """a second object on case B, for maps that the shared one must not see"""
    raw, _, _ = R.boundary_case()
    return _tl(raw, params[0], params[1])


def _class_of(kc, ne):
    return 0 if (kc <= 256 and ne <= 4096) else 1 if kc <= 1024 else 2 if kc <= 3840 else 3


@pytest.mark.parametrize('params', R.B_PARAMS)
def test_a_cell_alone_gives_the_bits_it_gives_among_the_others(gpu_device, params):
    """Each of the seven boundary cells of case B refitted with every other row in no cell: the LDS of a launch is sized by the
    largest cell of its class and the scratch and the results are slices of shared arrays, none of which may show in a cell's fit."""
    _, full, zfull, _ = _boundary_fit(params)
    raw, cor, _ = R.boundary_case()
    tl = _boundary_scratch(params)
    n_cells = len(R.B_CELLS)
    for c in range(7):
        alone = np.where(cor == c, cor, -1).astype(np.int32)
        fits = tl.em_cells(alone, n_cells, use_likelihood=params[2])
        want = [0, 0, 0, 0]
        want[0] += n_cells - 1                               # (the cells without rows are classed as wave cells)
        want[_class_of(*R.B_CELLS[c])] += 1
        assert _classes(tl._eng) == tuple(want), (c, _classes(tl._eng), want)
        _assert_same_cell(_cell(fits, c), _cell(full, c), ('alone', params, c))
        z = _z_aligned(tl)
        mine = _entries_of(raw, np.flatnonzero(cor == c))
        assert _same_bits(z[mine], zfull[mine]), ('alone', params, c)
        other = np.ones(len(z), bool)
        other[mine] = False
        assert np.all(z[other] == -1.0), ('alone', params, c)   # (the export's mark for `not in z's pattern`)


@pytest.mark.parametrize('params', R.B_PARAMS)
def test_a_permutation_of_the_cell_ids_permutes_the_fits(gpu_device, params):
    _, full, zfull, classes = _boundary_fit(params)
    raw, cor, _ = R.boundary_case()
    tl = _boundary_scratch(params)
    n_cells = len(R.B_CELLS)
    perm = np.random.RandomState(4).permutation(n_cells).astype(np.int32)
    assert not np.array_equal(perm, np.arange(n_cells))
    fits = tl.em_cells(perm[cor], n_cells, use_likelihood=params[2])
    assert _classes(tl._eng) == classes
    for c in range(n_cells):
        _assert_same_cell(_cell(fits, perm[c]), _cell(full, c), ('permuted', params, c))
    assert _same_bits(_z_aligned(tl), zfull), ('permuted', params)


# ---- c. repeated calls and the cached layout ----------------------------------------------------------------------------------------
def _second_map(n, seed=31, n_cells=55):
    """another map of shape 1's rows: more cells (so another total of compacted columns), other rows left out"""
    rng = np.random.RandomState(seed)
    cor = rng.randint(0, n_cells, n).astype(np.int32)
    cor[rng.rand(n) < 0.2] = -1
    return cor, n_cells


def test_repeated_calls_on_one_object(gpu_device):
    """The layout is cached per group map and the result buffers live as long as it does: a second call with the same map, a call with
    another map (more cells, another total Kc) in between, a map set by `reassign_cell_counts` in between, one iteration only and
    back — every fit equals, bit for bit, the fit of a fresh object; the pooled fit stays what it was."""
    raw, cor_a, n_a, ref = R.shape_case(1)
    cor_b, n_b = _second_map(raw.shape[0])
    fresh_a, fresh_b = _tl(raw), _tl(raw)
    want_a = fresh_a.em_cells(cor_a, n_a)
    want_b = fresh_b.em_cells(cor_b, n_b)
    za, zb = _z_aligned(fresh_a), _z_aligned(fresh_b)
    assert want_a.n_cells != want_b.n_cells and want_a.col_ptr[-1] != want_b.col_ptr[-1]
    _check_fits(want_a, ref, 'fresh A')

    tl = _tl(raw)
    pooled = dict(pi=tl.pi.copy(), theta=tl.theta.copy(), lnl=tl.lnl, n_iter=tl.n_iter, dev=tl._eng.get_params(1))

    def pooled_untouched(label):
        assert _same_bits(tl.pi, pooled['pi']) and _same_bits(tl.theta, pooled['theta']), label
        assert tl.lnl == pooled['lnl'] and tl.n_iter == pooled['n_iter'], label
        pi, theta = tl._eng.get_params(1)
        assert _same_bits(pi, pooled['dev'][0]) and _same_bits(theta, pooled['dev'][1]), label

    _assert_same_fit(tl.em_cells(cor_a, n_a), _z_aligned(tl), want_a, za, 'first A')
    _assert_same_fit(tl.em_cells(cor_a, n_a), _z_aligned(tl), want_a, za, 'A again')
    pooled_untouched('A, A')
    _assert_same_fit(tl.em_cells(cor_b, n_b), _z_aligned(tl), want_b, zb, 'B after A')
    _assert_same_fit(tl.em_cells(cor_a, n_a), _z_aligned(tl), want_a, za, 'A after B')
    pooled_untouched('A, B, A')
    tl.reassign_cell_counts('exclude', cor_b, n_b)           # another map between two fits
    _assert_same_fit(tl.em_cells(cor_a, n_a), _z_aligned(tl), want_a, za, 'A after the counts of B')

    tl.max_iter = 1
    one = tl.em_cells(cor_a, n_a)
    fitted = np.asarray([om is not None for om in ref.fits])
    assert fitted.all()
    assert np.all(one.n_iter == 1) and not np.any(one.converged)
    assert _same_bits(one.pi, one.pi_init) and _same_bits(one.theta, one.theta_init)
    assert _same_bits(one.pi_init, want_a.pi_init) and _same_bits(one.theta_init, want_a.theta_init)
    ref1 = R.cell_ref('shape1', 0, 200000, False, 1)
    _check_fits(one, ref1, 'max_iter 1')
    _check_z(tl, ref1, 'max_iter 1')
    pooled_untouched('max_iter 1')
    tl.max_iter = R.MAX_ITER
    _assert_same_fit(tl.em_cells(cor_a, n_a), _z_aligned(tl), want_a, za, 'A at 100 iterations again')
    pooled_untouched('the end')


# ---- d. engine options ----------------------------------------------------------------------------------------------------------------
def _option_matrix(which):
    if which == 'shape1':
        raw, cor, n_cells, _ = R.shape_case(1)
        return raw, cor, n_cells
    return R.large_case()


@functools.lru_cache(maxsize=None)
def _default_engine_fit(which):
    raw, cor, n_cells = _option_matrix(which)
    tl = _tl(raw)
    fits = tl.em_cells(cor, n_cells)
    info = tl._eng.layout_info()
    info['csr_indices_bytes'] = tl._eng.device_memory()['resident']['csr_indices']
    return fits, _z_aligned(tl), info


def _option_taken(options, info, default):
    """the engine really runs the layout asked for (as tests/test_gpu_rowpass_entries.py asserts it)"""
    for key, v in options.items():
        if key == 'value_format':
            assert info['value_bytes'] == (2 if v == 2 else 8) and (v != 2 or info['fused'] == 1), (options, info)
        if key == 'hot_split':
            assert info['hot_cols'] == 0, (options, info)
        if key == 'split':
            assert info['split'] == 1, (options, info)
        if key == 'parts':
            assert info['P'] == v, (options, info)
        if key == 'reproducible':
            assert info['reproducible'] >= 1 and default['reproducible'] == 0, (options, info)


@pytest.mark.parametrize('options', OPTION_SETS, ids=lambda o: '-'.join('%s%d' % kv for kv in o.items()))
@pytest.mark.parametrize('which', ['shape1', 'large'])
def test_engine_options_do_not_show_in_the_fits(gpu_device, which, options):
    """The unit reads the CSR codes, the score table and the row statistics only: under every layout of the pooled engine the fits
    and z have the default engine's bits.  Shape 1 has wave and 256-thread cells; `large` the 512-thread cell of the largest LDS launch
    (Kc = 3840) and a workspace cell (3841).  With `drop_csr_indices` the column ids are rebuilt for the set-up and go again."""
    raw, cor, n_cells = _option_matrix(which)
    want, zwant, default = _default_engine_fit(which)
    if which == 'shape1':
        _check_fits(want, R.shape_case(1)[3], 'shape 1, default engine')
        assert default['cell_em_wave'] > 0 and default['cell_em_256'] > 0
    else:
        _check_fits(want, R.cell_ref('large', 0, 200000), 'large, default engine')
        assert tuple(default[n] for n in CLASS_NAMES) == (0, 0, 1, 1)
    tl = _tl(raw, options=options)
    info = tl._eng.layout_info()
    _option_taken(options, info, default)
    if options.get('drop_csr_indices'):
        assert default['csr_indices_bytes'] >= 4 * raw.nnz and tl._eng.device_memory()['resident']['csr_indices'] == 0
    fits = tl.em_cells(cor, n_cells)
    if options.get('drop_csr_indices'):                      # (before anything else could drop them again)
        assert tl._eng.device_memory()['resident']['csr_indices'] == 0, 'the column ids stayed resident after the per-cell fit'
    _assert_same_fit(fits, _z_aligned(tl), want, zwant, (which, options))
    assert _classes(tl._eng) == tuple(default[n] for n in CLASS_NAMES)


# ---- e. degenerate cells ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('priors', PRIORS)
def test_rows_without_entries_and_a_cell_made_of_them(gpu_device, priors):
    """Five rows of a 300 x 40 matrix have no stored entries: three sit in otherwise normal cells (class 0, weight 0: they change
    nothing), two are a cell of their own (Kc = 0).  The oracle gives that cell NaN pi and theta everywhere — 0 / 0 in both closed
    forms —, 100 iterations, not converged, lnl 0.0; the device must agree, and the cell owns no z."""
    raw, cor, n_cells = R.empty_rows_case()
    ref = R.cell_ref('empty_rows', *priors)
    om = ref.fits[6]
    assert np.sum(np.diff(raw.indptr) == 0) == 5 and len(ref.rows[6]) == 2 and raw[ref.rows[6]].nnz == 0
    assert np.all(np.isnan(om.pi)) and np.all(np.isnan(om.theta)) and om.n_iter == R.MAX_ITER and not om.converged and om.lnl == 0.0
    tl = _tl(raw, *priors)
    fits = tl.em_cells(cor, n_cells)
    _check_fits(fits, ref, ('empty rows', priors))
    _check_z(tl, ref, ('empty rows', priors))
    assert fits.col_ptr[7] == fits.col_ptr[6] and fits.n_iter[6] == R.MAX_ITER and not fits.converged[6] and fits.lnl[6] == 0.0
    assert all(np.all(np.isnan(v)) for v in fits.dense(6)[:2])
    assert sp.csr_matrix(tl.z)[ref.rows[6]].nnz == 0


@pytest.mark.parametrize('priors', PRIORS)
def test_a_cell_that_touches_every_column(gpu_device, priors):
    """Kc == K: no `rest` column exists, and none may count in diff."""
    raw, cor, n_cells = R.full_columns_case()
    ref = R.cell_ref('full_columns', *priors)
    tl = _tl(raw, *priors)
    fits = tl.em_cells(cor, n_cells)
    assert fits.col_ptr[1] - fits.col_ptr[0] == raw.shape[1] == 64
    _check_fits(fits, ref, ('Kc = K', priors))
    _check_z(tl, ref, ('Kc = K', priors))


@pytest.mark.parametrize('priors', PRIORS)
@pytest.mark.parametrize('K', [2, 1])
def test_one_and_two_columns(gpu_device, K, priors):
    """K of 2 and 1 through the engine-level path (the pooled layouts need min(shape) >= 8; the engine loads such a matrix).  At
    theta_prior = 0 the oracle gives NaN theta at K = 1 (one iteration, converged, lnl NaN), and NaN pi and theta for the cell of
    unique rows at K = 2 (100 iterations, not converged, lnl NaN): the device reproduces n_iter, converged and the NaN pattern."""
    raw, cor, n_cells = R.tiny_k_case(K)
    ref = R.cell_ref('K%d' % K, *priors)
    if priors == (0, 0):
        if K == 1:
            assert all(om.n_iter == 1 and om.converged and np.isnan(om.lnl) and np.all(np.isnan(om.theta)) for om in ref.fits)
        else:
            om = ref.fits[1]
            assert om.n_iter == R.MAX_ITER and not om.converged and np.isnan(om.lnl) and np.all(np.isnan(om.theta)) and np.any(np.isnan(om.pi))
    got = _EngineFit(gpu_device, raw, cor, n_cells, *priors)
    _check_fits(got.fits, ref, ('K', K, priors))
    for c, om in enumerate(ref.fits):
        for mine, theirs in zip(got.fits.dense(c), (om.pi, om.theta, om.pi_init, om.theta_init)):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (K, priors, c)
        assert np.isnan(got.fits.lnl[c]) == np.isnan(om.lnl), (K, priors, c)
    _check_z(got, ref, ('K', K, priors))


# ---- f. no pooled fit before the per-cell fits ----------------------------------------------------------------------------------------
def test_no_pooled_fit_is_needed(gpu_device):
    """Shape 3 through the engine-level path, `cell_em` straight after `set_groups`: the bits of the fit with a pooled em() first."""
    n, k, n_cells, theta_prior, pi_prior, use_lnl = R.SHAPES[3]
    raw, cor, _, ref = R.shape_case(3)
    got = _EngineFit(gpu_device, raw, cor, n_cells, pi_prior, theta_prior, use_lnl)
    tl = _tl(raw, pi_prior, theta_prior)
    want = tl.em_cells(cor, n_cells, use_likelihood=use_lnl)
    _assert_same_fit(got.fits, got.z_aligned, want, _z_aligned(tl), 'no pooled fit')
    _check_fits(got.fits, ref, 'no pooled fit')
    _check_z(got, ref, 'no pooled fit')
