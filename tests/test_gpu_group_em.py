"""The SPREAD class of the per-group EM fits (tsem_cell_em with engine option "cell_em_spread_entries": a group with more stored
entries is fitted by the whole grid, one set of short launches per iteration) and `sc --pooling_mode celltype` on top of it.

The yardstick is the oracle run per group (tests/_cell_em_reference.py: RTOL = 1e-9, atol 0, iteration counts equal; tests/
test_celltype_host.py asserts that none of the counts compared here hinges on a rounding); what is stated as identical is compared as
bits.  Spreading is forced with the option at 1 — every group with more than one stored entry — or put between the sizes of a case's
groups.  Every reference is computed once per session (shared with tests/test_gpu_cell_em*.py where the case is theirs)."""
import functools
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
import _cell_em_reference as R
import _group_em_reference as GR
from _cell_em_reference import ALL_METHODS, INT_METHODS, RTOL, _check_fits, _check_z

pytestmark = pytest.mark.gpu
GOLDEN = GR.GOLDEN
FIT_ARRAYS = ('col_ptr', 'cols', 'pi', 'theta', 'pi_init', 'theta_init', 'rest', 'n_iter', 'converged', 'lnl')
COLUMN_ARRAYS = ('cols', 'pi', 'theta', 'pi_init', 'theta_init')
CELL_ARRAYS = ('rest', 'n_iter', 'converged', 'lnl')
CLASS_NAMES = ('cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _tl(raw, pi_prior=0, theta_prior=200000, spread=1, options=None, pooled_iters=5, max_iter=R.MAX_ITER):
    """A fresh object with a pooled fit (a few iterations: it only has to exist) and the spread option set."""
    from telescope_amd.likelihood import TelescopeLikelihood
    eo = dict(options or {})
    eo['cell_em_spread_entries'] = spread
    tl = TelescopeLikelihood(raw, Opts(pi_prior=pi_prior, theta_prior=theta_prior, max_iter=pooled_iters), engine_options=eo)
    tl.em()
    tl.max_iter = max_iter
    return tl


def _z_aligned(tl_or_eng):
    from telescope_amd import _lib
    return getattr(tl_or_eng, '_eng', tl_or_eng).export_z(_lib.Z_USER)


def _counts(tl_or_eng):
    """(spread, (wave, 256, 512, global)) of the last fit"""
    info = getattr(tl_or_eng, '_eng', tl_or_eng).layout_info()
    return info['cell_em_spread'], tuple(info[n] for n in CLASS_NAMES)


def _entries(raw, cor, n):
    raw = sp.csr_matrix(raw)
    lens = np.diff(raw.indptr)
    keep = np.asarray(cor) >= 0
    return np.bincount(np.asarray(cor)[keep], weights=lens[keep], minlength=n).astype(np.int64)


def _old_class(raw, cor, c):
    sub = sp.csr_matrix(raw)[np.flatnonzero(np.asarray(cor) == c)]
    k, e = len(np.unique(sub.indices)), sub.nnz
    return 0 if (k <= 256 and e <= 4096) else 1 if k <= 1024 else 2 if k <= 3840 else 3


def _want_counts(raw, cor, n, threshold):
    """by the documented rule, from the matrix alone"""
    ne = _entries(raw, cor, n)
    old = [0, 0, 0, 0]
    spread = 0
    for c in range(n):
        if threshold > 0 and ne[c] > threshold:
            spread += 1
        else:
            old[_old_class(raw, cor, c)] += 1
    return spread, tuple(old)


def _cell(fits, c):
    a, b = int(fits.col_ptr[c]), int(fits.col_ptr[c + 1])
    out = {name: getattr(fits, name)[a:b] for name in COLUMN_ARRAYS}
    out.update({name: getattr(fits, name)[c] for name in CELL_ARRAYS})
    return out


def _assert_same_cell(got, want, label):
    for name in COLUMN_ARRAYS + CELL_ARRAYS:
        assert _same_bits(got[name], want[name]), (label, name, got[name], want[name])


def _assert_same_fit(a, za, b, zb, label):
    for name in FIT_ARRAYS:
        assert _same_bits(getattr(a, name), getattr(b, name)), (label, name)
    assert _same_bits(za, zb), (label, 'z')


def _entries_of(raw, rows):
    return np.flatnonzero(np.isin(np.repeat(np.arange(raw.shape[0]), np.diff(raw.indptr)), rows))


class _EngineFit(object):
    """The engine-level path, no TelescopeLikelihood and no pooled fit; `.z` from the Z_USER export."""

    def __init__(self, device, raw, cor, n_cells, pi_prior, theta_prior, use_likelihood=False, spread=1):
        from telescope_amd import _lib
        from telescope_amd.likelihood import CellFits, score_lut
        raw = sp.csr_matrix(raw)
        self.eng = eng = _lib.Engine(device)
        eng.set_option('cell_em_spread_entries', spread)
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], score_lut(int(raw.max())))
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, pi_prior, theta_prior)
        eng.set_groups(cor, n_cells)
        r = eng.cell_em(R.EPSILON, R.MAX_ITER, use_likelihood)
        self.fits = CellFits(raw.shape[1], *[r[k] for k in CellFits.FIELDS])
        self.z_aligned = eng.export_z(_lib.Z_USER)
        keep = self.z_aligned >= 0
        rid = np.repeat(np.arange(raw.shape[0]), np.diff(raw.indptr))
        self.z = sp.csr_matrix((self.z_aligned[keep], (rid[keep], raw.indices[keep])), shape=raw.shape)


# ---- the option and the counter -----------------------------------------------------------------------------------------------
def test_option_and_layout_info(gpu_device):
    from telescope_amd import _lib
    eng = _lib.Engine(gpu_device)
    info = eng.layout_info()
    assert list(info)[33:38] == list(CLASS_NAMES) + ['cell_em_spread'] and len(info) == 40 and info['cell_em_spread'] == 0
    eng.set_option('cell_em_spread_entries', 0)
    eng.set_option('cell_em_spread_entries', 1 << 40)
    with pytest.raises(_lib.EngineError):
        eng.set_option('cell_em_spread_entries', -1)
    eng.close()


# ---- oracle parity --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shape_fit(seed):
    n, k, n_cells, theta_prior, pi_prior, use_lnl = R.SHAPES[seed]
    raw, cor, _, _ = R.shape_case(seed)
    tl = _tl(raw, pi_prior, theta_prior)
    before = dict(pi=tl.pi.copy(), theta=tl.theta.copy(), lnl=tl.lnl, n_iter=tl.n_iter, exclude=tl.reassign_colsums('exclude'),
                  dev=tl._eng.get_params(1))
    fits = tl.em_cells(cor, n_cells, use_likelihood=use_lnl)
    return tl, fits, before, _counts(tl)


@pytest.mark.parametrize('seed', [1, 3, 4, 5])
def test_spread_fits_equal_the_oracle_per_group(gpu_device, seed):
    """Shapes 1, 3, 4, 5 with every group spread: 1 has groups that stop at different iterations inside one launch sequence, 3 is the
    NaN-theta case, 4 has a pi prior and use_likelihood, 5 columns beyond every LDS class."""
    tl, fits, _, (spread, old) = _shape_fit(seed)
    raw, cor, n_cells, ref = R.shape_case(seed)
    with_entries = int(np.sum(_entries(raw, cor, n_cells) > 0))
    assert np.all(_entries(raw, cor, n_cells)[_entries(raw, cor, n_cells) > 0] > 1)
    print('shape %d spread: iterations %s' % (seed, sorted(set(fits.n_iter.tolist()))))
    assert spread == with_entries and old == (n_cells - with_entries, 0, 0, 0), (spread, old)
    if seed == 1:
        assert len(set(fits.n_iter.tolist())) > 3
    _check_fits(fits, ref, ('spread', seed))
    _check_z(tl, ref, ('spread', seed))


# ---- column tiers and row chunks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('params', GR.TIER_PARAMS)
def test_columns_at_the_edges_of_the_tiers(gpu_device, params):
    """Columns of exactly L | L + 1 entries (one lane | a wave), 64 m | 64 m + 1 of the wave tier, 4096 | 4097 (a wave | the
    workgroup) and 256 m | 256 m + 1 of the workgroup tier (tests/_group_em_reference.py: TIER_GROUPS), alone in their groups."""
    raw, cor, n = GR.tier_case()
    ref = GR.group_ref('tiers', *params)
    tl = _tl(raw, params[0], params[1])
    fits = tl.em_cells(cor, n, use_likelihood=params[2])
    assert _counts(tl) == (n, (0, 0, 0, 0))
    _check_fits(fits, ref, ('tiers', params))
    _check_z(tl, ref, ('tiers', params))


def test_groups_of_one_chunk_of_rows_one_more_and_one_row(gpu_device):
    raw, cor, n = GR.chunk_case()
    ref = GR.group_ref('chunks', 0, 200000)
    tl = _tl(raw)
    fits = tl.em_cells(cor, n)
    assert _counts(tl) == (3, (0, 0, 0, 0))
    _check_fits(fits, ref, 'chunks')
    _check_z(tl, ref, 'chunks')
    tl.max_iter = 1                                          # (and by the likelihood, one iteration: the lnl of one chunk + 1 row)
    ref1 = R.CellRef(raw, cor, n, 0, 200000, max_iter=1, use_likelihood=True)
    one = tl.em_cells(cor, n, use_likelihood=True)
    _check_fits(one, ref1, 'chunks, lnl')
    _check_z(tl, ref1, 'chunks, lnl')


# ---- mixed classes in one call -----------------------------------------------------------------------------------------------------
B_THRESHOLD = 3500                                         # between the sizes of case B's cells: 4096, 4097, 8000 | 3000, 40, 2, 1


@functools.lru_cache(maxsize=None)
def _mixed_fit(params):
    raw, cor, _ = R.boundary_case()
    tl = _tl(raw, params[0], params[1], spread=B_THRESHOLD)
    fits = tl.em_cells(cor, len(R.B_CELLS), use_likelihood=params[2])
    return tl, fits, _z_aligned(tl), _counts(tl)


@pytest.mark.parametrize('params', R.B_PARAMS)
def test_spread_and_one_workgroup_groups_in_one_call(gpu_device, params):
    """Case B with the threshold between its cells' sizes: five groups spread, five in their old classes; the oracle's fits; every
    group bit-identical to the same group fitted alone in the same class, and the groups that are not spread bit-identical to a fit
    with the option at 0."""
    raw, cor, _ = R.boundary_case()
    n = len(R.B_CELLS)
    tl, fits, z, counts = _mixed_fit(params)
    is_spread = np.asarray([ne > B_THRESHOLD for _, ne in R.B_CELLS])
    assert counts == _want_counts(raw, cor, n, B_THRESHOLD) == (5, (3, 1, 1, 0)) and is_spread.sum() == 5, counts
    ref = R.cell_ref('B', *params)
    _check_fits(fits, ref, ('mixed', params))
    _check_z(tl, ref, ('mixed', params))
    # the option at 0: nothing is spread, and the groups below the threshold have the same bits
    off = _tl(raw, params[0], params[1], spread=0)
    fits0 = off.em_cells(cor, n, use_likelihood=params[2])
    z0 = _z_aligned(off)
    assert _counts(off) == (0, R.B_CLASSES)
    changed = 0
    for c in range(n):
        mine = _entries_of(raw, np.flatnonzero(cor == c))
        if not is_spread[c]:
            _assert_same_cell(_cell(fits, c), _cell(fits0, c), ('option 0', params, c))
            assert _same_bits(z[mine], z0[mine]), ('option 0', params, c)
        else:
            changed += not all(_same_bits(_cell(fits, c)[k], _cell(fits0, c)[k]) for k in ('pi', 'theta', 'lnl'))
    print('case B %s: %d of 5 spread groups differ in bits from their one-workgroup fit' % (params, changed))
    # alone, same option: the same class, the same bits
    for c in (0, 2, 3, 6, 8):
        alone = np.where(cor == c, cor, -1).astype(np.int32)
        got = tl.em_cells(alone, n, use_likelihood=params[2])
        assert _counts(tl)[0] == int(is_spread[c]), (c, _counts(tl))
        _assert_same_cell(_cell(got, c), _cell(fits, c), ('alone', params, c))
        za = _z_aligned(tl)
        mine = _entries_of(raw, np.flatnonzero(cor == c))
        assert _same_bits(za[mine], z[mine]), ('alone', params, c)
        other = np.ones(len(za), bool)
        other[mine] = False
        assert np.all(za[other] == -1.0), ('alone', params, c)
    tl.em_cells(cor, n, use_likelihood=params[2])            # (leave the shared object as it was)


# ---- one arithmetic under both launch strategies ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('params', R.B_PARAMS)
def test_spread_has_the_one_workgroup_bits_where_the_orders_of_sums_coincide(gpu_device, params):
    """One group of 177 rows, 300 compacted columns and 600 entries, two per column at most: in the 256-thread LDS class, and one
    chunk of rows, a row per thread at most, two columns per thread at most, every column in the one-lane tier — so every sum of the
    spread class (the chunks' parts, the columns, diff, lnl) is taken in the one-workgroup class's order, and what is left to differ
    is the arithmetic of a row and of a column: the two classes share it, bit for bit."""
    raw, cor, _ = R.boundary_matrix(51, 2000, [(300, 600)])
    per_column = GR.column_counts(raw, cor, 0)
    n_rows = int(np.sum(cor == 0))
    assert (n_rows, len(per_column), raw.nnz, max(per_column)) == (177, 300, 600, 2) and n_rows == raw.shape[0]
    assert _old_class(raw, cor, 0) == 1                                                # 256 threads, the tables in LDS
    assert n_rows <= GR.SP_ROWS and n_rows <= GR.SP_T                                  # one chunk; a row per thread at most
    assert len(per_column) <= 2 * GR.SP_T and max(per_column) <= GR.SP_LANE            # two columns per thread; one lane per column
    one, spread = [_EngineFit(gpu_device, raw, cor, 1, params[0], params[1], params[2], spread=s) for s in (0, 1)]
    assert _counts(one.eng) == (0, (0, 1, 0, 0)) and _counts(spread.eng) == (1, (0, 0, 0, 0))
    print('one order %s: %d iterations, lnl %r' % (params, int(one.fits.n_iter[0]), float(one.fits.lnl[0])))
    _assert_same_fit(one.fits, one.z_aligned, spread.fits, spread.z_aligned, ('one order', params))
    one.eng.close()
    spread.eng.close()


# ---- determinism, twins, the host's looks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [1, 4])
def test_two_spread_runs_on_fresh_objects_are_bit_identical(gpu_device, seed):
    tl_a, fits_a, _, _ = _shape_fit(seed)
    n, k, n_cells, theta_prior, pi_prior, use_lnl = R.SHAPES[seed]
    raw, cor, _, _ = R.shape_case(seed)
    tl_b = _tl(raw, pi_prior, theta_prior)
    fits_b = tl_b.em_cells(cor, n_cells, use_likelihood=use_lnl)
    _assert_same_fit(fits_a, _z_aligned(tl_a), fits_b, _z_aligned(tl_b), ('two runs', seed))


def test_twin_columns_of_a_spread_group_have_identical_parameters(gpu_device):
    raw, cor, n = GR.twin_case()
    ref = GR.group_ref('twins2', 0, 200000)
    tl = _tl(raw)
    fits = tl.em_cells(cor, n)
    assert _counts(tl) == (2, (0, 0, 0, 0))
    _check_fits(fits, ref, 'twins')
    n_classes = 0
    for c in range(n):
        dense = fits.dense(c)
        for cols in ref.twin_classes(c):
            n_classes += 1
            for v, name in zip(dense, ('pi', 'theta', 'pi_init', 'theta_init')):
                assert len(set(_bits(v[cols]).tolist())) == 1, (c, cols, name)
    assert n_classes > 100


@functools.lru_cache(maxsize=None)
def _tier_fit():
    raw, cor, n = GR.tier_case()
    tl = _tl(raw)
    return tl, tl.em_cells(cor, n)


@pytest.mark.parametrize('max_iter', GR.LOOK_ITERS)
@pytest.mark.parametrize('which', ['tiers', 'shape3'])
def test_the_hosts_looks_do_not_show(gpu_device, which, max_iter):
    """max_iter 1, 7, 8, 9 around the host's look at the done marks every 8 iterations, on the tier case (the oracle stops its groups
    after 4, 5 and 9 iterations) and shape 3 (8, 9, 10, ... 100): the oracle's fits at that max_iter, and a group that stops before
    max_iter has the bits of the run bounded by 100 iterations."""
    if which == 'tiers':
        raw, cor, n_cells = GR.tier_case()
        priors = (0, 200000)
        full = _tier_fit()[1]
    else:
        raw, cor, n_cells, _ = R.shape_case(3)
        priors = (0, 0)
        full = _shape_fit(3)[1]
    ref = GR.group_ref(which, priors[0], priors[1], False, max_iter)
    tl = _tl(raw, *priors, max_iter=max_iter)
    fits = tl.em_cells(cor, n_cells)
    _check_fits(fits, ref, (which, 'max_iter', max_iter))
    _check_z(tl, ref, (which, 'max_iter', max_iter))
    assert fits.n_iter.max() == max_iter
    early = np.flatnonzero((full.n_iter < max_iter) & (full.n_iter > 0))
    assert (len(early) > 0) == (max_iter > (4 if which == 'tiers' else 8)), (which, max_iter, len(early))
    for c in early:
        _assert_same_cell(_cell(fits, c), _cell(full, c), (which, 'max_iter', max_iter, c))


# ---- degenerate groups, spread forced ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('priors', GR.DEGENERATE_PRIORS)
def test_degenerate_groups_beside_spread_ones(gpu_device, priors):
    """Rows without entries inside spread groups and a group made of such rows only (Kc = 0: not spread, it has no entries); a group
    that touches every column (Kc = K: no `rest` column counts in diff); a group without rows."""
    raw, cor, n = R.empty_rows_case()
    ref = R.cell_ref('empty_rows', *priors)
    tl = _tl(raw, *priors)
    fits = tl.em_cells(cor, n)
    assert _counts(tl) == (6, (1, 0, 0, 0))
    _check_fits(fits, ref, ('empty rows', priors))
    _check_z(tl, ref, ('empty rows', priors))
    assert fits.col_ptr[7] == fits.col_ptr[6] and fits.n_iter[6] == R.MAX_ITER and not fits.converged[6]
    raw, cor, n = R.full_columns_case()
    ref = R.cell_ref('full_columns', *priors)
    tl = _tl(raw, *priors)
    fits = tl.em_cells(cor, n + 1)                           # (group 2 has no rows)
    assert _counts(tl) == (2, (1, 0, 0, 0)) and fits.col_ptr[1] - fits.col_ptr[0] == raw.shape[1]
    assert fits.n_iter[2] == 0 and not fits.converged[2] and np.isnan(fits.lnl[2])
    for c in range(n):
        om = ref.fits[c]
        assert fits.n_iter[c] == om.n_iter and bool(fits.converged[c]) == bool(om.converged), (priors, c)
        for got, want in zip(fits.dense(c), (om.pi, om.theta, om.pi_init, om.theta_init)):
            assert np.allclose(got, want, rtol=RTOL, atol=0, equal_nan=True), (priors, c)
        assert np.isclose(fits.lnl[c], om.lnl, rtol=RTOL, atol=0, equal_nan=True), (priors, c)
    _check_z(tl, ref, ('Kc = K', priors))


@pytest.mark.parametrize('priors', GR.DEGENERATE_PRIORS)
@pytest.mark.parametrize('K', [2, 1])
def test_one_and_two_columns_spread(gpu_device, K, priors):
    raw, cor, n = R.tiny_k_case(K)
    ref = R.cell_ref('K%d' % K, *priors)
    got = _EngineFit(gpu_device, raw, cor, n, *priors)
    assert _counts(got.eng) == _want_counts(raw, cor, n, 1) and _counts(got.eng)[0] >= 1
    _check_fits(got.fits, ref, ('K', K, priors))
    for c, om in enumerate(ref.fits):
        for mine, theirs in zip(got.fits.dense(c), (om.pi, om.theta, om.pi_init, om.theta_init)):
            assert np.array_equal(np.isnan(mine), np.isnan(theirs)), (K, priors, c)
        assert np.isnan(got.fits.lnl[c]) == np.isnan(om.lnl), (K, priors, c)
    _check_z(got, ref, ('K', K, priors))
    got.eng.close()


def test_no_pooled_fit_is_needed_for_spread_groups(gpu_device):
    n, k, n_cells, theta_prior, pi_prior, use_lnl = R.SHAPES[3]
    raw, cor, _, ref = R.shape_case(3)
    got = _EngineFit(gpu_device, raw, cor, n_cells, pi_prior, theta_prior, use_lnl)
    tl, want, _, counts = _shape_fit(3)
    assert _counts(got.eng) == counts
    _assert_same_fit(got.fits, got.z_aligned, want, _z_aligned(tl), 'no pooled fit')
    _check_z(got, ref, 'no pooled fit')
    got.eng.close()


# ---- the pooled state, engine options ------------------------------------------------------------------------------------------------------
def test_pooled_state_is_untouched_by_spread_fits(gpu_device):
    tl, fits, before, _ = _shape_fit(1)
    assert _same_bits(tl.pi, before['pi']) and _same_bits(tl.theta, before['theta'])
    assert tl.lnl == before['lnl'] and tl.n_iter == before['n_iter']
    pi, theta = tl._eng.get_params(1)
    assert _same_bits(pi, before['dev'][0]) and _same_bits(theta, before['dev'][1])
    cells = tl.reassign_colsums('exclude')
    tl.select_z('pooled')
    try:
        assert np.array_equal(tl.reassign_colsums('exclude'), before['exclude'])
        assert not np.array_equal(cells, before['exclude'])
    finally:
        tl.select_z('cells')
    assert np.array_equal(tl.reassign_colsums('exclude'), cells)


def test_drop_csr_indices_keeps_working(gpu_device):
    raw, cor, n_cells, _ = R.shape_case(1)
    tl_w, want, _, counts = _shape_fit(1)
    tl = _tl(raw, options={'drop_csr_indices': 1})
    assert tl._eng.device_memory()['resident']['csr_indices'] == 0
    fits = tl.em_cells(cor, n_cells)
    assert tl._eng.device_memory()['resident']['csr_indices'] == 0, 'the column ids stayed resident after the fit'
    assert _counts(tl) == counts
    _assert_same_fit(fits, _z_aligned(tl), want, _z_aligned(tl_w), 'drop_csr_indices')


# ---- two maps: the fit under the types, the counts under the barcodes ------------------------------------------------------------------------
def _two_maps(case, spread, seed, methods):
    raw, cor, tor, ref, n_types = case
    n_cells = int(cor.max()) + 1
    tl = _tl(raw, spread=spread)
    fits = tl.em_cells(tor, n_types)
    _check_fits(fits, ref, 'two maps')
    z = _z_aligned(tl)
    und = ref.undecided_rows()
    cor2 = np.where(tor >= 0, cor, -1).astype(np.int32)      # (a barcode without type counts nowhere)
    cor2[und] = -1
    S = R.selector(cor2, n_cells)
    om = ref.pooled_model()
    for method in methods:
        np.random.seed(seed)
        got = tl.reassign_cell_counts(method, cor2, n_cells, 0.9).toarray()
        np.random.seed(seed)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            want = (S @ sp.csr_matrix(om.reassign(method, 0.9)).astype(np.float64)).toarray()
        if method in INT_METHODS:
            assert np.array_equal(got, want), (method, int(np.sum(got != want)))
        else:
            assert np.allclose(got, want, rtol=RTOL, atol=1e-12), (method, np.max(np.abs(got - want)))
        assert _same_bits(_z_aligned(tl), z), ('the Z_USER buffer of the fit went with the barcode map', method)
    return tl, fits, z


@pytest.mark.parametrize('spread', [1, 0])
def test_counts_under_the_barcode_map_after_a_fit_under_the_type_map(gpu_device, spread):
    """`reassign_cell_counts` under the barcode map reads the z of the fit under the type map: for every method the counts equal
    selector(barcodes) @ oracle.reassign(method) — integer methods exactly outside the rows the oracle cannot decide itself, `average`
    and `conf` at RTOL — and the Z_USER buffer stays what the fit left.  `choose` where every tie is a twin tie (both sides then draw
    for the same rows); the other five on shape 1 as well."""
    tl, fits, z = _two_maps(GR.two_maps_twin_case(), spread, 5, ALL_METHODS)
    assert _counts(tl)[0] == (4 if spread else 0)
    raw, cor, tor, ref, n_types = GR.two_maps_case()
    tl, fits, z = _two_maps(GR.two_maps_case(), spread, 1, [m for m in ALL_METHODS if m != 'choose'])
    assert _counts(tl)[0] == (5 if spread else 0)
    # the barcodes without type: in no group, no posterior, rows of zeros — under the barcodes' own map as well
    n_cells = int(cor.max()) + 1
    counts = tl.reassign_cell_counts('all', np.where(tor >= 0, cor, -1).astype(np.int32), n_cells)
    assert counts[3].nnz == 0 and counts[17].nnz == 0 and counts[0].nnz > 0
    rows = np.flatnonzero(tor < 0)
    assert np.all(z[_entries_of(raw, rows)] == -1.0)
    # and a fit under the barcode map afterwards is what it is on a fresh object
    again = tl.em_cells(tor, n_types)
    _assert_same_fit(again, _z_aligned(tl), fits, z, 'type map again')


# ---- end to end ----------------------------------------------------------------------------------------------------------------------------
def _sc_run(argv, outdir):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _check_celltype_files(outdir, ts, tor, ref, wants):
    import pandas as pd
    tag = os.path.join(str(outdir), 'telescope-')
    names = sorted(ts.feat_index, key=ts.feat_index.get)
    omitted = list(ts.barcodes).index(GR.E2E_OMITTED)
    for method in ALL_METHODS:
        got = pd.read_csv(tag + 'TE_counts_%s.tsv' % method, sep='\t', index_col=0)
        assert list(got.index) == list(ts.barcodes) and list(got.columns) == names, method
        assert np.all(got.values[omitted] == 0), method
        if method in INT_METHODS:
            assert np.array_equal(got.values, wants[method]), method
        else:
            assert np.allclose(got.values, wants[method], rtol=RTOL, atol=1e-12), method
    lines = open(tag + 'celltype_stats.tsv').read().splitlines()
    assert lines[0].split('\t') == ['celltype', 'cells', 'fragments', 'ambiguous', 'columns', 'iterations', 'converged', 'lnl']
    assert len(lines) == 1 + len(GR.E2E_TYPES)
    cor = np.asarray(ts.cell_of_row)
    for t, line in enumerate(lines[1:]):
        f = line.split('\t')
        om = ref.fits[t]
        assert f[0] == GR.E2E_TYPES[t] and int(f[1]) == len(set(cor[tor == t].tolist())) and int(f[2]) == len(ref.rows[t])
        assert int(f[3]) == int(om.Y.sum()) and int(f[4]) == len(np.unique(ref.raw[ref.rows[t]].indices))
        assert int(f[5]) == om.n_iter and f[6] == str(bool(om.converged))
        assert np.isclose(float(f[7]), om.lnl, rtol=RTOL, atol=0)
    assert not os.path.exists(tag + 'cell_stats.tsv')


def test_sc_assign_and_resume_with_celltype_pooling(gpu_device, tmp_path):
    """`sc assign --pooling_mode celltype` on the fixture with tests/golden/sc_mixed_celltypes.tsv — four of the five barcodes in two
    types, one left out, one barcode the run does not contain — and `sc resume` of its checkpoint: the per-barcode tables of all six
    methods against the oracle built the same way, EVERY row of every barcode (the fixture's ties are exact on both sides:
    tests/test_celltype_host.py), the omitted barcode's row all zero, the two lines of celltype_stats.tsv, run_stats.tsv untouched."""
    from telescope_amd.run_container import scTelescope
    bam, gtf = os.path.join(GOLDEN, 'sc_mixed.bam'), os.path.join(GOLDEN, 'sc_mixed.gtf')
    mode = ['--pooling_mode', 'celltype', '--celltype_tsv', GR.E2E_TSV]
    _sc_run(['sc', 'assign', bam, gtf] + mode + ['--use_every_reassign_mode'], tmp_path / 'a')
    ckpt = str(tmp_path / 'a' / 'telescope-checkpoint.npz')
    ts = scTelescope.load(ckpt)
    tor, ref = GR.e2e_reference(ts)
    n_cells = len(ts.barcodes)
    om = ref.pooled_model()
    S = R.selector(np.where(tor >= 0, ts.cell_of_row, -1), n_cells)
    np.random.seed(ts.get_random_seed())                     # (`choose` is the run's only draw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        wants = {m: (S @ sp.csr_matrix(om.reassign(m, 0.9)).astype(np.float64)).toarray() for m in ('conf', 'all', 'unique', 'exclude', 'choose', 'average')}
    _check_celltype_files(tmp_path / 'a', ts, tor, ref, wants)
    assert open(str(tmp_path / 'a' / 'telescope-run_stats.tsv')).read() == open(os.path.join(GOLDEN, 'sc_ref-run_stats.tsv')).read()
    _sc_run(['sc', 'resume', ckpt] + mode + ['--use_every_reassign_mode'], tmp_path / 'r')
    _check_celltype_files(tmp_path / 'r', ts, tor, ref, wants)
    for name in ['TE_counts_%s.tsv' % m for m in ALL_METHODS] + ['celltype_stats.tsv', 'run_stats.tsv']:
        assert open(str(tmp_path / 'a' / ('telescope-' + name))).read() == open(str(tmp_path / 'r' / ('telescope-' + name))).read(), name
    _sc_run(['sc', 'resume', ckpt] + mode + ['--count_format', 'mtx'], tmp_path / 'm')
    import scipy.io
    m = scipy.io.mmread(str(tmp_path / 'm' / 'telescope-TE_counts.mtx')).toarray()
    assert np.array_equal(m, wants['exclude'])
