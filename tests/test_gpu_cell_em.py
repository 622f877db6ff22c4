"""Per-cell EM fits on the device (`TelescopeLikelihood.em_cells`, tsem_cell_em) against the oracle run once per cell on the cell's
rows with the score scale of the whole matrix: iteration counts, parameters, lnl and z per cell; determinism; exact twins; the
pooled state left alone; the per-cell count matrices of all six methods; and `sc assign --pooling_mode individual` end to end.

Shapes (tests/_cell_em_reference.py): 1-5 are the random matrices the feature was specified with — 2 and 3 are all small cells (a wave
per cell), 1 mixes them with the 256-thread class that 4 takes throughout, 5 the global-workspace class (Kc ~ 5900 > 3840) — and 6 adds the 512-thread LDS
class (Kc ~ 2400).  Every reference is computed once per session and shared."""
import functools
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
import _cell_em_reference as R
from _cell_em_reference import ALL_METHODS, INT_METHODS, RTOL, _check_fits, _check_z

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SEEDS = sorted(R.SHAPES)
FIT_ARRAYS = ('col_ptr', 'cols', 'pi', 'theta', 'pi_init', 'theta_init', 'rest', 'n_iter', 'converged', 'lnl')


def _tl(raw, pi_prior=0, theta_prior=200000, pooled_iters=100):
    from telescope_amd.likelihood import TelescopeLikelihood
    tl = TelescopeLikelihood(raw, Opts(pi_prior=pi_prior, theta_prior=theta_prior, max_iter=pooled_iters))
    tl.em()
    tl.max_iter = R.MAX_ITER
    return tl


def _fit_shape(seed):
    """A fresh object: pooled fit (20 iterations: it only has to exist), then the per-cell fits."""
    n, k, n_cells, theta_prior, pi_prior, use_lnl = R.SHAPES[seed]
    raw, cor = R.random_matrix(seed, n, k, n_cells)
    tl = _tl(raw, pi_prior, theta_prior, pooled_iters=20)
    before = dict(pi=tl.pi.copy(), theta=tl.theta.copy(), lnl=tl.lnl, n_iter=tl.n_iter, exclude=tl.reassign_colsums('exclude'))
    fits = tl.em_cells(cor, n_cells, use_likelihood=use_lnl)
    return tl, fits, before


@functools.lru_cache(maxsize=None)
def _device_case(seed):
    return _fit_shape(seed)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize('seed', SEEDS)
def test_fits_equal_the_oracle_per_cell(gpu_device, seed):
    tl, fits, _ = _device_case(seed)
    ref = R.shape_case(seed)[3]
    _check_fits(fits, ref, seed)
    _check_z(tl, ref, seed)


def test_every_class_is_exercised(gpu_device):
    """The shapes reach all four cell classes: a wave per cell, 256 threads, 512 threads (LDS), global workspace — by the cells'
    column counts, and by the counts per class the unit itself reports for each shape's fit (`layout_info`: every cell of the map is
    classed, one without rows as a wave cell)."""
    kc = {seed: np.diff(_device_case(seed)[1].col_ptr) for seed in SEEDS}
    assert kc[2].max() <= 256
    assert 256 < kc[4].min() and kc[4].max() <= 1024
    assert 1024 < kc[6].min() and kc[6].max() <= 3840
    assert kc[5].min() > 3840
    names = ('cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global')
    got = {}
    for seed in SEEDS:
        info = _device_case(seed)[0]._eng.layout_info()
        got[seed] = tuple(info[n] for n in names)
    assert got[2] == (200, 0, 0, 0) and got[3] == (25, 0, 0, 0), got
    assert got[4] == (0, 30, 0, 0) and got[6] == (0, 0, 4, 0) and got[5] == (0, 0, 0, 3), got
    raw, cor, n_cells, ref = R.shape_case(1)                 # shape 1 by the documented rule, from the matrix alone
    want = [0, 0, 0, 0]
    for rows in ref.rows:
        sub = raw[rows]
        k, e = len(np.unique(sub.indices)), sub.nnz
        want[0 if (k <= 256 and e <= 4096) else 1 if k <= 1024 else 2 if k <= 3840 else 3] += 1
    assert got[1] == tuple(want) and want[0] > 0 and want[1] > 0 and want[2] == want[3] == 0, (got[1], want)
    from telescope_amd import _lib
    fresh = _lib.Engine(gpu_device)
    assert all(fresh.layout_info()[n] == 0 for n in names)   # 0 before a fit
    fresh.close()


@pytest.mark.parametrize('seed', SEEDS)
def test_two_runs_on_fresh_objects_are_bit_identical(gpu_device, seed):
    tl_a, fits_a, _ = _device_case(seed)
    tl_b, fits_b, _ = _fit_shape(seed)
    for name in FIT_ARRAYS:
        assert _same_bits(getattr(fits_a, name), getattr(fits_b, name)), (seed, name)
    za, zb = sp.csr_matrix(tl_a.z), sp.csr_matrix(tl_b.z)
    assert np.array_equal(za.indptr, zb.indptr) and np.array_equal(za.indices, zb.indices) and _same_bits(za.data, zb.data), seed


@pytest.mark.parametrize('seed', SEEDS)
def test_twin_columns_of_a_cell_have_identical_parameters(gpu_device, seed):
    _, fits, _ = _device_case(seed)
    ref = R.shape_case(seed)[3]
    n_classes = 0
    for c in range(ref.n_cells):
        if ref.fits[c] is None:
            continue
        dense = fits.dense(c)
        for cols in ref.twin_classes(c):
            n_classes += 1
            for v, name in zip(dense, ('pi', 'theta', 'pi_init', 'theta_init')):
                assert len(set(_bits(v[cols]).tolist())) == 1, (seed, c, cols, name)
    if seed == 2:
        assert n_classes > 100                               # (small cells: a read on two loci nobody else hits is the common case)


def test_pooled_state_is_untouched(gpu_device):
    tl, fits, before = _device_case(1)
    assert _same_bits(tl.pi, before['pi']) and _same_bits(tl.theta, before['theta'])
    assert tl.lnl == before['lnl'] and tl.n_iter == before['n_iter']
    pi, theta = tl._eng.get_params(1)
    assert _same_bits(pi, before['pi']) and _same_bits(theta, before['theta'])
    cells = tl.reassign_colsums('exclude')
    tl.select_z('pooled')
    try:
        assert np.array_equal(tl.reassign_colsums('exclude'), before['exclude'])
        assert not np.array_equal(cells, before['exclude'])   # (the per-cell z is another z)
    finally:
        tl.select_z('cells')
    assert np.array_equal(tl.reassign_colsums('exclude'), cells)
    with pytest.raises(ValueError):
        tl.select_z('other')


@pytest.mark.parametrize('seed', [1, 2, 4])
def test_cell_counts_under_the_per_cell_z(gpu_device, seed):
    tl, fits, _ = _device_case(seed)
    raw, cor, n_cells, ref = R.shape_case(seed)
    # first reference: scipy's sum of the device's own reassign matrix, bit for bit
    S = R.selector(cor, n_cells)
    for method in ALL_METHODS:
        np.random.seed(seed)
        got = tl.reassign_cell_counts(method, cor, n_cells, 0.9)
        np.random.seed(seed)
        want = (S @ tl.reassign(method, 0.9).tocsr().astype(np.float64)).tocsr()
        want.sort_indices()
        assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices) \
            and _same_bits(got.data, want.data), (seed, method)
    # second reference: the oracle's reassign of the assembled per-cell z, without the rows it cannot decide itself
    und = ref.undecided_rows()
    print('shape %d: %d of %d fitted rows left out of the comparison with the oracle' % (seed, len(und), ref.fitted_rows()))
    assert len(und) <= 0.005 * ref.fitted_rows(), (len(und), ref.fitted_rows())
    cor2 = cor.copy()
    cor2[und] = -1
    S2 = R.selector(cor2, n_cells)
    om = ref.pooled_model()
    for method in ALL_METHODS:
        if method == 'choose':                               # (against the oracle only where both sides draw for the same rows: below)
            continue
        got = tl.reassign_cell_counts(method, cor2, n_cells, 0.9).toarray()
        want = (S2 @ sp.csr_matrix(om.reassign(method, 0.9)).astype(np.float64)).toarray()
        if method in INT_METHODS:
            assert np.array_equal(got, want), (seed, method, int(np.sum(got != want)))
        else:
            assert np.allclose(got, want, rtol=RTOL, atol=1e-12), (seed, method, np.max(np.abs(got - want)))
    tl.reassign_cell_counts('all', cor, n_cells)             # (leave the shared object on the shape's own map)


def test_choose_equals_the_oracle_where_all_ties_are_twin_ties(gpu_device):
    raw, cor, n_cells = R.twin_tie_matrix()
    ref = R.CellRef(raw, cor, n_cells, 0, 200000)
    assert len(ref.undecided_rows()) == 0
    tl = _tl(raw, pooled_iters=5)
    fits = tl.em_cells(cor, n_cells)
    _check_fits(fits, ref, 'twin ties')
    _check_z(tl, ref, 'twin ties')
    om = ref.pooled_model()
    S = R.selector(cor, n_cells)
    tied = int(np.sum(np.diff(raw.indptr) == 2))
    assert tied > 200
    for method in ALL_METHODS:
        np.random.seed(5)
        got = tl.reassign_cell_counts(method, cor, n_cells, 0.9).toarray()
        np.random.seed(5)
        want = (S @ sp.csr_matrix(om.reassign(method, 0.9)).astype(np.float64)).toarray()
        if method in INT_METHODS:
            assert np.array_equal(got, want), method
        else:
            assert np.allclose(got, want, rtol=RTOL, atol=1e-12), method
    assert tl.reassign_cell_counts('exclude', cor, n_cells).nnz < tl.reassign_cell_counts('choose', cor, n_cells).nnz


def test_hand_made_partition(gpu_device):
    """An empty cell, a one-row cell, a cell of unique rows only — theta = NaN at theta_prior = 0, as the closed form gives — and a
    cell with everything else."""
    raw, _ = R.random_matrix(7, 600, 80, 4)
    lens = np.diff(raw.indptr)
    cor = np.full(raw.shape[0], 3, np.int32)
    cor[np.flatnonzero(lens > 1)[0]] = 1                     # cell 1: one (ambiguous) row
    cor[np.flatnonzero(lens == 1)[:150]] = 2                 # cell 2: unique rows only
    cor[-20:] = -1                                           # cell 0 stays empty
    ref = R.CellRef(raw, cor, 4, 0, 0)
    assert ref.fits[0] is None and np.all(np.isnan(ref.fits[2].theta)) and ref.fits[2].n_iter == R.MAX_ITER
    tl = _tl(raw, 0, 0, pooled_iters=10)
    fits = tl.em_cells(cor, 4)
    _check_fits(fits, ref, 'hand-made')
    assert np.all(np.isnan(fits.dense(2)[1]))
    _check_z(tl, ref, 'hand-made')
    cells = tl.reassign_cell_counts('all', cor, 4)
    assert cells[0].nnz == 0 and cells[2].nnz == 0           # (cell 2: every z is NaN, no entry counts)


@pytest.mark.parametrize('use_likelihood', [False, True])
def test_all_rows_in_one_cell_is_the_pooled_fit(gpu_device, use_likelihood):
    from telescope_amd.likelihood import TelescopeLikelihood
    raw, _ = R.random_matrix(8, 4000, 700, 1)
    tl = TelescopeLikelihood(raw, Opts(pi_prior=1 if use_likelihood else 0, use_likelihood=use_likelihood))
    tl.em(use_likelihood=use_likelihood)
    pooled_z = sp.csr_matrix(tl.z)
    fits = tl.em_cells(np.zeros(tl.N, np.int32), 1, use_likelihood=use_likelihood)
    assert fits.n_iter[0] == tl.n_iter and bool(fits.converged[0]) == bool(tl.converged)
    pi, theta, pi_init, theta_init = fits.dense(0)
    for got, want in ((pi, tl.pi), (theta, tl.theta), (pi_init, tl.pi_init), (theta_init, tl.theta_init)):
        assert np.allclose(got, want, rtol=RTOL, atol=0)
    assert np.isclose(fits.lnl[0], tl.lnl, rtol=RTOL, atol=0)
    z = sp.csr_matrix(tl.z)
    assert np.array_equal(z.indptr, pooled_z.indptr) and np.array_equal(z.indices, pooled_z.indices)
    assert np.allclose(z.data, pooled_z.data, rtol=RTOL, atol=0)


def test_argument_checks_on_the_device(gpu_device):
    from telescope_amd import _lib
    raw, cor = R.random_matrix(9, 300, 40, 5)
    tl = _tl(raw, pooled_iters=3)
    with pytest.raises(ValueError):
        tl.select_z('cells')                                 # no per-cell fit yet
    with pytest.raises(ValueError):
        tl.em_cells(cor[:-1], 5)
    with pytest.raises(ValueError):
        tl.em_cells(cor, 3)
    tl._eng.set_groups(None, 0)
    with pytest.raises(_lib.EngineError):
        tl._eng.cell_em(1e-7, 100)                           # no group map
    fits = tl.em_cells(cor, 5)
    tl.z = sp.csr_matrix(tl.z)                               # a caller's z replaces the device buffer
    tl.reassign_colsums('exclude')
    with pytest.raises(ValueError):
        tl.select_z('cells')
    assert fits.n_cells == 5


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _sc_run(argv, outdir):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def _check_individual_files(outdir, ts, ref, wants):
    import pandas as pd
    tag = os.path.join(str(outdir), 'telescope-')
    names = sorted(ts.feat_index, key=ts.feat_index.get)
    for method in ALL_METHODS:
        got = pd.read_csv(tag + 'TE_counts_%s.tsv' % method, sep='\t', index_col=0)
        assert list(got.index) == list(ts.barcodes) and list(got.columns) == names, method
        if method in INT_METHODS:
            assert np.array_equal(got.values, wants[method]), method
        else:
            assert np.allclose(got.values, wants[method], rtol=RTOL, atol=1e-12), method
    lines = open(tag + 'cell_stats.tsv').read().splitlines()
    assert lines[0].split('\t') == ['barcode', 'fragments', 'ambiguous', 'columns', 'iterations', 'converged', 'lnl']
    assert len(lines) == 1 + len(ts.barcodes)
    for c, line in enumerate(lines[1:]):
        f = line.split('\t')
        om = ref.fits[c]
        assert f[0] == ts.barcodes[c] and int(f[1]) == len(ref.rows[c])
        assert int(f[2]) == int(om.Y.sum()) and int(f[3]) == len(np.unique(ref.raw[ref.rows[c]].indices))
        assert int(f[4]) == om.n_iter and f[5] == str(bool(om.converged))
        assert np.isclose(float(f[6]), om.lnl, rtol=RTOL, atol=0)


def test_sc_assign_and_resume_with_individual_pooling(gpu_device, tmp_path):
    from telescope_amd.run_container import scTelescope
    bam, gtf = os.path.join(GOLDEN, 'sc_mixed.bam'), os.path.join(GOLDEN, 'sc_mixed.gtf')
    _sc_run(['sc', 'assign', bam, gtf, '--pooling_mode', 'individual', '--use_every_reassign_mode'], tmp_path / 'a')
    ckpt = str(tmp_path / 'a' / 'telescope-checkpoint.npz')
    ts = scTelescope.load(ckpt)
    raw = sp.csr_matrix(ts.raw_scores)
    n_cells = len(ts.barcodes)
    ref = R.CellRef(raw, ts.cell_of_row, n_cells, 0, 200000)
    assert all(om is not None for om in ref.fits)
    om = ref.pooled_model()
    S = R.selector(ts.cell_of_row, n_cells)
    np.random.seed(ts.get_random_seed())                     # (`choose` is the run's only draw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        wants = {m: (S @ sp.csr_matrix(om.reassign(m, 0.9)).astype(np.float64)).toarray() for m in ('conf', 'all', 'unique', 'exclude', 'choose', 'average')}
    _check_individual_files(tmp_path / 'a', ts, ref, wants)
    assert open(str(tmp_path / 'a' / 'telescope-run_stats.tsv')).read() == open(os.path.join(GOLDEN, 'sc_ref-run_stats.tsv')).read()
    _sc_run(['sc', 'resume', ckpt, '--pooling_mode', 'individual', '--use_every_reassign_mode'], tmp_path / 'r')
    _check_individual_files(tmp_path / 'r', ts, ref, wants)
    for name in ['TE_counts_%s.tsv' % m for m in ALL_METHODS] + ['cell_stats.tsv', 'run_stats.tsv']:
        assert open(str(tmp_path / 'a' / ('telescope-' + name))).read() == open(str(tmp_path / 'r' / ('telescope-' + name))).read(), name
    _sc_run(['sc', 'resume', ckpt, '--pooling_mode', 'individual', '--count_format', 'mtx'], tmp_path / 'm')
    import scipy.io
    m = scipy.io.mmread(str(tmp_path / 'm' / 'telescope-TE_counts.mtx')).toarray()
    assert np.array_equal(m, wants['exclude'])
    assert open(str(tmp_path / 'm' / 'telescope-barcodes.tsv')).read().split() == list(ts.barcodes)
