"""Per-group bootstrap on the device (`TelescopeLikelihood.bootstrap(..., cell_of_row=...)`, tsem_bootstrap_groups) against its
definition: every replicate's per-(group, column) values equal the oracle's reassign matrix of the replicate summed per group — equal
for exclude / unique / all, at RTOL for average / conf — on the structural pattern; mean and sd are numpy's over the good replicates;
the plain results are those of the plain call; a single-cell run's tables end to end.  Cases, references and fairness asserts are those of tests/test_gpu_bootstrap.py
(tests/_bootstrap_reference.py); the group maps come from a RandomState of this file's own (tests/_group_bootstrap_reference.py)."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
import _bootstrap_reference as B
import _group_bootstrap_reference as GB
from _bootstrap_reference import RTOL

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NREP = len(B.REPS)


def _tl(raw, pi_prior, theta_prior, device=0, max_iter=B.MAX_ITER, **engine_options):
    from telescope_amd.likelihood import TelescopeLikelihood
    return TelescopeLikelihood(raw, Opts(pi_prior=pi_prior, theta_prior=theta_prior, em_epsilon=B.EPSILON, max_iter=max_iter),
                               device=device, engine_options=engine_options or None)


@functools.lru_cache(maxsize=None)
def _case_tl(name):
    _, _, _, pp, tp = B.CASES[name]
    return _tl(B.case_matrix(name), pp, tp)


def _fair(ref):
    assert ref.undecided() == 0
    assert ref.stop_margin() > 1e-6, ref.stop_margin()


def _check_counts(fits, ref, method, label):
    for b, om in enumerate(ref.fits):
        if om is None:
            continue
        want = ref.counts(b, method)
        if method in B.INT_METHODS:
            assert np.array_equal(fits.counts[b], want), (label, method, b)
        else:
            assert np.allclose(fits.counts[b], want, rtol=RTOL, atol=0), (label, method, b)


def _check_pattern(cells, raw, cor, n_cells):
    gptr, cols = GB.structural_pattern(raw, cor, n_cells)
    assert cells.n_cells == n_cells and np.array_equal(cells.group_ptr, gptr) and np.array_equal(cells.cols, cols)
    assert cells.group_ptr.dtype == np.int64 and cells.cols.dtype == np.int32
    return gptr, cols


def _check_values(fits, ref, method, cor, n_cells, label, reps=None):
    """every kept replicate against the reference, through values_matrix and on the pattern; then mean / sd against numpy's moments
    of the kept values"""
    cells = fits.cells
    gptr, cols = cells.group_ptr, cells.cols
    good = np.array([om is not None and not np.isnan(om.lnl) for om in ref.fits])
    for b in (range(fits.n_rep) if reps is None else reps):
        if not good[b]:
            assert np.all(np.isnan(cells.values[b])), (label, b)
            continue
        want = GB.group_values(ref, b, method, cor, n_cells)
        got = cells.values_matrix(b)
        assert got.shape == (n_cells, ref.K)
        if method in B.INT_METHODS:
            assert np.array_equal(got.toarray(), want), (label, method, b)
            assert np.array_equal(cells.values[b], GB.on_pattern(want, gptr, cols)), (label, method, b)
        else:
            assert np.allclose(got.toarray(), want, rtol=RTOL, atol=0), (label, method, b)
    assert cells.n_used == int(good.sum()), (label, cells.n_used)
    wm, ws = GB.moments(cells.values, good)
    print('%s %s: %d slots, n_used %d, max mean %.6g' % (label, method, cells.nnz, cells.n_used, np.nanmax(np.abs(wm)) if cells.nnz else 0.))
    GB.assert_moments(cells.mean, cells.sd, wm, ws, (label, method))
    return good


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['C1', 'C2'])
def test_values_of_every_method_equal_the_oracle_per_group(gpu_device, name):
    """40 groups, a tenth of the rows in none; group 0, a middle group and group 39 are empty."""
    ref = B.case_ref(name)
    _fair(ref)
    raw, g = B.case_matrix(name), 40
    cor = GB.random_map(101, raw.shape[0], g, empty=(0, 17, 39))
    assert (cor < 0).any() and set(np.unique(cor[cor >= 0])) == set(range(g)) - {0, 17, 39}
    tl = _case_tl(name)
    for method in B.METHODS:
        fits = tl.bootstrap(NREP, seed=B.SEED, method=method, thresh=B.CONF, cell_of_row=cor, n_cells=g, keep_replicates=True)
        B.check_replicates(fits, ref, (name, method))
        _check_counts(fits, ref, method, name)
        gptr, _ = _check_pattern(fits.cells, raw, cor, g)
        assert gptr[1] == 0 and gptr[18] == gptr[17] and gptr[40] == gptr[39]
        _check_values(fits, ref, method, cor, g, name)
        assert fits.cells.n_used == NREP
        if method in B.INT_METHODS:                            # exact: the groups' values and the ungrouped rows' add up to the counts
            for b in range(NREP):
                assert np.array_equal(np.asarray(fits.cells.values_matrix(b).sum(0)).ravel() + GB.ungrouped_counts(ref, b, method, cor),
                                      fits.counts[b]), (name, method, b)


# 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_long_column_lists_take_many_search_steps(gpu_device):
    """C3: K = 1500, more columns than LDS slots; 3 groups, so a group's column list has several hundred entries."""
    ref = B.case_ref('C3')
    _fair(ref)
    raw = B.case_matrix('C3')
    cor = GB.random_map(102, raw.shape[0], 3)
    fits = _case_tl('C3').bootstrap(NREP, seed=B.SEED, method='exclude', cell_of_row=cor, n_cells=3, keep_replicates=True)
    gptr, _ = _check_pattern(fits.cells, raw, cor, 3)
    assert np.diff(gptr).min() >= 300, np.diff(gptr)
    B.check_replicates(fits, ref, 'C3')
    _check_counts(fits, ref, 'exclude', 'C3')
    _check_values(fits, ref, 'exclude', cor, 3, 'C3')


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_long_rows_and_a_full_batch_plus_one(gpu_device):
    """The long-rows matrix of test_gpu_bootstrap.py (seed 40): rows of up to 40 entries, 9 = 8 + 1 replicates, 16 hot columns,
    max_iter 30; 7 groups, `average`."""
    rng = np.random.RandomState(40)
    n, k = 1200, 300
    lens = rng.randint(1, 41, n)
    lens[rng.rand(n) < 0.3] = 1
    idx = []
    for l in lens:
        hot = rng.choice(16, min(l // 3, 16), replace=False)
        rest = 16 + rng.choice(k - 16, l - len(hot), replace=False)
        idx.append(np.sort(np.concatenate([hot, rest])))
    indptr = np.concatenate([[0], np.cumsum(lens)])
    raw = sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), np.concatenate(idx).astype(np.int32), indptr), shape=(n, k))
    mult = B.default_multiplicities(n, seed=5, reps=range(9))
    ref = B.BootRef(raw, mult, 0, 200000, max_iter=30)
    _fair(ref)
    cor = GB.random_map(103, n, 7)
    tl = _tl(raw, 0, 200000, device=gpu_device, max_iter=30, boot_hot_columns=16)
    fits = tl.bootstrap(9, seed=5, method='average', cell_of_row=cor, n_cells=7, keep_replicates=True)
    assert fits.info == {'batch': 8, 'hot_columns': 16}
    B.check_replicates(fits, ref, 'long rows')
    _check_counts(fits, ref, 'average', 'long rows')
    _check_pattern(fits.cells, raw, cor, 7)
    _check_values(fits, ref, 'average', cor, 7, 'long rows')
    assert fits.cells.n_used == 9


# 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_explicit_multiplicities_and_a_bad_replicate(gpu_device):
    """C2 with the replicates ones, zeros, zero on ambiguous rows, ten rows at 255: the zeros replicate is bad."""
    raw = B.case_matrix('C2')
    _, n, k, pp, tp = B.CASES['C2']
    rng = np.random.RandomState(3)
    mult = np.ones((4, n), np.uint8)
    mult[1] = 0
    mult[2, np.diff(raw.indptr) > 1] = 0
    mult[3, rng.choice(n, 10, replace=False)] = 255
    ref = B.BootRef(raw, mult, pp, tp)
    _fair(ref)
    g = 40
    cor = GB.random_map(101, n, g, empty=(0, 17, 39))
    fits = _case_tl('C2').bootstrap(4, method='exclude', multiplicities=mult, cell_of_row=cor, n_cells=g, keep_replicates=True)
    B.check_replicates(fits, ref, 'explicit')
    good = _check_values(fits, ref, 'exclude', cor, g, 'explicit')
    assert list(good) == [True, False, True, True] and fits.cells.n_used == 3
    assert fits.cells.nnz > 0 and np.all(np.isnan(fits.cells.values[1]))
    pooled = _tl(raw, pp, tp)
    pooled.em()
    want = pooled.reassign_cell_counts('exclude', cor, g)
    assert np.array_equal(fits.cells.values_matrix(0).toarray(), want.toarray())


# 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_group_of_every_row_and_no_group_at_all(gpu_device):
    ref = B.case_ref('C2')
    _fair(ref)
    raw = B.case_matrix('C2')
    tl = _case_tl('C2')
    one = np.zeros(raw.shape[0], np.int32)
    for method in ('exclude', 'all'):
        fits = tl.bootstrap(NREP, seed=B.SEED, method=method, cell_of_row=one, n_cells=1, keep_replicates=True)
        _check_pattern(fits.cells, raw, one, 1)
        for b in range(NREP):
            assert np.array_equal(fits.cells.values_matrix(b).toarray()[0], fits.counts[b]), (method, b)
        _check_counts(fits, ref, method, 'one group')
    none = np.full(raw.shape[0], -1, np.int32)
    fits = tl.bootstrap(NREP, seed=B.SEED, method='exclude', cell_of_row=none, n_cells=3, keep_replicates=True)
    c = fits.cells
    assert c.nnz == 0 and np.array_equal(c.group_ptr, [0, 0, 0, 0]) and c.values.shape == (NREP, 0) and c.n_used == NREP
    assert c.mean_matrix().shape == (3, raw.shape[1]) and c.mean_matrix().nnz == 0 and c.sd_matrix().nnz == 0 and c.values_matrix(2).nnz == 0
    B.check_replicates(fits, ref, 'no group')
    _check_counts(fits, ref, 'exclude', 'no group')


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_no_good_replicate_gives_nan_statistics_on_the_pattern(gpu_device):
    """The unique-only matrix at theta_prior = 0: every replicate's parameters are NaN."""
    rng = np.random.RandomState(5)
    n, k = 300, 20
    raw = sp.csr_matrix((rng.randint(100, 400, n).astype(np.uint16), (np.arange(n), rng.randint(0, k, n))), shape=(n, k))
    cor = GB.random_map(104, n, 6)
    fits = _tl(raw, 0, 0).bootstrap(2, seed=B.SEED, cell_of_row=cor, n_cells=6, keep_replicates=True)
    assert np.isnan(fits.counts).all() and np.isnan(fits.lnl).all() and not fits.fitted.any()
    c = fits.cells
    _check_pattern(c, raw, cor, 6)
    assert c.n_used == 0 and c.nnz > 0
    assert np.isnan(c.mean).all() and np.isnan(c.sd).all() and np.isnan(c.values).all()


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_memory_and_column_id_paths_give_the_same_results(gpu_device):
    from telescope_amd import _lib
    raw = B.case_matrix('C2')
    _, _, _, pp, tp = B.CASES['C2']
    ref = B.case_ref('C2')
    _fair(ref)
    g = 40
    cor = GB.random_map(101, raw.shape[0], g, empty=(0, 17, 39))
    kw = dict(seed=B.SEED, method='exclude', cell_of_row=cor, n_cells=g, keep_replicates=True)
    base = _case_tl('C2').bootstrap(NREP, **kw)
    assert base.info['batch'] == NREP
    slots = base.cells.nnz
    for opts, batch in (({'boot_batch': 2}, 2), ({'boot_group_bytes': 8 * slots * 2 + 7}, 2), ({'boot_group_bytes': 8 * slots}, 1),
                        ({'drop_csr_indices': 1}, NREP),
                        # the pattern built in many tiles of a few groups (2048 entries), and with groups beyond a tile (128 entries)
                        ({'group_tile_bytes': 1 << 16}, NREP), ({'group_tile_bytes': 1 << 12}, NREP)):
        tl = _tl(raw, pp, tp, **opts)
        if 'drop_csr_indices' in opts:
            assert tl._eng.device_memory()['resident']['csr_indices'] == 0
        fits = tl.bootstrap(NREP, **kw)
        if 'drop_csr_indices' in opts:
            assert tl._eng.device_memory()['resident']['csr_indices'] == 0
        assert fits.info['batch'] == batch, (opts, fits.info)
        B.check_replicates(fits, ref, tuple(opts.items()))
        _check_counts(fits, ref, 'exclude', tuple(opts.items()))
        assert np.array_equal(fits.cells.group_ptr, base.cells.group_ptr) and np.array_equal(fits.cells.cols, base.cells.cols)
        assert np.array_equal(fits.cells.values, base.cells.values), opts
        assert np.array_equal(fits.cells.mean, base.cells.mean) and np.array_equal(fits.cells.sd, base.cells.sd), opts
    tl = _tl(raw, pp, tp, boot_group_bytes=8 * slots - 1)
    with pytest.raises(_lib.EngineError, match='boot_group_bytes') as e:
        tl.bootstrap(NREP, **kw)
    assert e.value.code == _lib.ERR_NOMEM and str(8 * slots) in str(e.value)
    with pytest.raises(_lib.EngineError):
        tl._eng.set_option('boot_group_bytes', -1)


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_statistics_do_not_depend_on_keeping_the_values(gpu_device):
    raw = B.case_matrix('C1')
    cor = GB.random_map(101, raw.shape[0], 40, empty=(0, 17, 39))
    tl = _case_tl('C1')
    kept = tl.bootstrap(NREP, seed=B.SEED, method='exclude', cell_of_row=cor, n_cells=40, keep_replicates=True)
    lean = tl.bootstrap(NREP, seed=B.SEED, method='exclude', cell_of_row=cor, n_cells=40)
    assert lean.cells.values is None and kept.cells.values.shape == (NREP, kept.cells.nnz)
    assert np.array_equal(lean.cells.mean, kept.cells.mean) and np.array_equal(lean.cells.sd, kept.cells.sd)
    assert np.array_equal(lean.cells.cols, kept.cells.cols) and lean.cells.n_used == kept.cells.n_used == NREP
    assert np.array_equal(lean.counts, kept.counts)
    with pytest.raises(ValueError):
        lean.cells.values_matrix(0)


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone_and_the_plain_call_is_unchanged(gpu_device):
    raw = B.case_matrix('C2')
    _, _, _, pp, tp = B.CASES['C2']
    ref = B.case_ref('C2')
    tl = _tl(raw, pp, tp)
    tl.em()
    z = sp.csr_matrix(tl.z)
    before = (tl.pi.copy(), tl.theta.copy(), tl.lnl, tl.n_iter, z.data.copy(), z.indices.copy(), tl.reassign_colsums('exclude'))
    plain = tl.bootstrap(NREP, seed=B.SEED)
    assert plain.cells is None
    g = 40
    cor = GB.random_map(101, raw.shape[0], g, empty=(0, 17, 39))
    counts_before = tl.reassign_cell_counts('exclude', cor, g).toarray()
    fits = tl.bootstrap(NREP, seed=B.SEED, cell_of_row=cor, n_cells=g)
    B.check_replicates(fits, ref, 'grouped')
    tl._z = None                                               # export z from the device again
    tl._report_cache = {}
    z2 = sp.csr_matrix(tl.z)
    pi2, theta2 = tl._eng.get_params(1)
    assert np.array_equal(before[0].view(np.uint64), pi2.view(np.uint64)) and np.array_equal(before[1].view(np.uint64), theta2.view(np.uint64))
    assert np.array_equal(before[0], tl.pi) and before[2] == tl.lnl and before[3] == tl.n_iter
    assert np.array_equal(before[4].view(np.uint64), z2.data.view(np.uint64)) and np.array_equal(before[5], z2.indices)
    assert np.array_equal(before[6], tl.reassign_colsums('exclude'))
    again = tl.bootstrap(NREP, seed=B.SEED)
    assert again.cells is None and again.info == plain.info
    assert np.array_equal(plain.n_iter, again.n_iter) and np.array_equal(plain.converged, again.converged)
    assert np.array_equal(plain.n_frags, again.n_frags) and np.array_equal(plain.counts, again.counts)
    assert np.allclose(plain.pi, again.pi, rtol=RTOL, atol=0) and np.allclose(plain.theta, again.theta, rtol=RTOL, atol=0)
    assert np.allclose(plain.lnl, again.lnl, rtol=RTOL, atol=0)
    assert np.array_equal(fits.counts, plain.counts) and np.array_equal(fits.n_iter, plain.n_iter)
    assert np.array_equal(tl.reassign_cell_counts('exclude', cor, g).toarray(), counts_before)
    cor2 = GB.random_map(105, raw.shape[0], 9, none=0.5)
    other = tl.bootstrap(NREP, seed=B.SEED, cell_of_row=cor2, n_cells=9, keep_replicates=True)
    _check_pattern(other.cells, raw, cor2, 9)
    assert other.cells.nnz != fits.cells.nnz
    _check_values(other, ref, 'exclude', cor2, 9, 'second map')
    back = tl.bootstrap(NREP, seed=B.SEED, cell_of_row=cor, n_cells=g)   # ... and the first map again
    assert np.array_equal(back.cells.cols, fits.cells.cols) and np.array_equal(back.cells.mean, fits.cells.mean)
    assert np.array_equal(back.cells.sd, fits.cells.sd)


# 10 --------------------------------------------------------------------------------------------------------------------------------
def test_engine_refusals(gpu_device):
    from telescope_amd import _lib
    raw = B.case_matrix('C2')
    _, _, k, pp, tp = B.CASES['C2']
    tl = _tl(raw, pp, tp)
    with pytest.raises(_lib.EngineError, match='group map') as e:     # no group map
        tl._eng.bootstrap_groups(2, 0, None, 'exclude', 0.9, 1e-7, 10, k)
    assert e.value.code == _lib.ERR_ARG
    cor = GB.random_map(101, raw.shape[0], 5)
    tl._eng.set_groups(cor, 5)
    with pytest.raises(_lib.EngineError, match='choose') as e:
        tl._eng.bootstrap_groups(2, 0, None, 'choose', 0.9, 1e-7, 10, k)
    assert e.value.code == _lib.ERR_ARG
    rep = _tl(raw, pp, tp, reproducible=1)
    rep._eng.set_groups(cor, 5)
    with pytest.raises(_lib.EngineError, match='reproducible') as e:
        rep._eng.bootstrap_groups(2, 0, None, 'exclude', 0.9, 1e-7, 10, k)
    assert e.value.code == _lib.ERR_ARG
    with pytest.raises(ValueError, match='choose'):
        tl.bootstrap(2, method='choose', cell_of_row=cor, n_cells=5)
    with pytest.raises(ValueError):
        tl.bootstrap(2, cell_of_row=cor)                       # n_cells is needed
    with pytest.raises(ValueError):
        tl.bootstrap(2, cell_of_row=cor[:-1], n_cells=5)


# 11 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fmt', ['tsv', 'mtx'])
def test_sc_run_with_bootstrap_tables_end_to_end(gpu_device, tmp_path, fmt):
    """tests/golden/sc_mixed.bam through the single-cell container: the ordinary report, then ONE bootstrap(8, seed 3,
    cell_of_row=...) call gives bootstrap.tsv and the mean / sd tables — with the count table's shape and labels, beside files that are
    byte-identical to a run without them, and with the numbers of a fresh model on the written checkpoint."""
    import types
    import pandas as pd
    import scipy.io
    from telescope_amd.likelihood import TelescopeLikelihood
    from telescope_amd.loader import Annotation
    from telescope_amd.run_container import scTelescope

    def run(outdir, boot):
        os.makedirs(str(outdir))
        opts = types.SimpleNamespace(samfile=os.path.join(GOLDEN, 'sc_mixed.bam'), no_feature_key='__no_feature', overlap_mode='threshold',
                                     overlap_threshold=0.2, stranded_mode='None', barcode_tag='CB', updated_sam=False,
                                     reassign_mode='exclude', conf_prob=0.9, count_format=fmt, use_every_reassign_mode=False,
                                     pooling_mode='pseudobulk', em_epsilon=1e-7, max_iter=100, pi_prior=0, theta_prior=200000,
                                     outfile_path=lambda suffix: os.path.join(str(outdir), 'telescope-' + suffix))
        ts = scTelescope(opts)
        ts.load_alignment(Annotation(os.path.join(GOLDEN, 'sc_mixed.gtf'), 'locus', 'None'))
        ts.save(opts.outfile_path('checkpoint'))
        np.random.seed(ts.get_random_seed())
        tl = TelescopeLikelihood(ts.raw_scores, opts, device=gpu_device)
        tl.em()
        ts.output_report(tl, opts.outfile_path('run_stats.tsv'), opts.outfile_path('TE_counts.tsv'))
        if boot:
            fits = tl.bootstrap(8, 3, method='exclude', thresh=0.9, cell_of_row=ts.cell_of_row, n_cells=len(ts.barcodes))
            ts.output_bootstrap(tl, fits, opts.outfile_path('bootstrap.tsv'), 0.9)
            ts.output_cell_bootstrap(fits, opts.outfile_path('TE_counts_boot_mean.tsv'), opts.outfile_path('TE_counts_boot_sd.tsv'))
    plain, boot = tmp_path / 'plain', tmp_path / 'boot'
    run(plain, False)
    run(boot, True)
    was = sorted(os.listdir(str(plain)))
    table = 'telescope-TE_counts.' + fmt
    assert 'telescope-checkpoint.npz' in was and table in was and 'telescope-run_stats.tsv' in was
    new = ['telescope-bootstrap.tsv', 'telescope-TE_counts_boot_mean.' + fmt, 'telescope-TE_counts_boot_sd.' + fmt]
    assert sorted(os.listdir(str(boot))) == sorted(was + new)
    for name in was:
        if name.endswith('.npz'):                              # (an archive carries the time it was written: its members are compared)
            a, b = np.load(str(plain / name)), np.load(str(boot / name))
            assert sorted(a.files) == sorted(b.files) and all(np.array_equal(a[f], b[f]) for f in a.files)
        else:
            assert (plain / name).read_bytes() == (boot / name).read_bytes(), name
    head = (boot / 'telescope-bootstrap.tsv').read_text().splitlines()[0].split('\t')
    assert head[0] == '## Bootstrap' and 'replicates:8' in head and 'seed:3' in head and 'fitted:8' in head and 'level:0.9' in head

    def read(name):
        if fmt == 'tsv':
            t = pd.read_csv(str(boot / name), sep='\t', index_col=0, float_precision='round_trip')   # (the writer prints repr)
            return t.values, list(t.index), list(t.columns)
        return scipy.io.mmread(str(boot / name)).toarray(), None, None
    counts, rows, cols = read(table)
    mean, mrows, mcols = read(new[1])
    sd, srows, scols = read(new[2])
    assert mean.shape == sd.shape == counts.shape and (mrows, mcols) == (srows, scols) == (rows, cols)
    assert np.all(sd >= 0) and np.all(mean >= 0)
    ts = scTelescope.load(str(boot / 'telescope-checkpoint.npz'))
    tl = TelescopeLikelihood(ts.raw_scores, Opts(), device=gpu_device)
    fits = tl.bootstrap(8, 3, method='exclude', thresh=0.9, cell_of_row=ts.cell_of_row, n_cells=len(ts.barcodes))
    assert fits.cells.n_used == 8 and counts.shape == (len(ts.barcodes), tl.K)
    assert np.array_equal(mean, fits.cells.mean_matrix().toarray()) and np.array_equal(sd, fits.cells.sd_matrix().toarray())
    if fmt == 'tsv':
        assert rows == list(ts.barcodes)
