"""Single-cell mode on the device: the sparse per-cell count matrix (tsem_group_counts / reassign_cell_counts) against
scipy's sum of the device's own `reassign` matrix — bit-identical for every method, the float-valued `average` and `conf`
included — against the oracle, through every layout, on edge-case partitions and at droplet scale; and `sc assign` /
`sc resume` end to end against files the reference wrote."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts, case_matrix, case_names, load_case

pytestmark = pytest.mark.gpu
RTOL = 1e-9
ALL_METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')
INT_METHODS = ('exclude', 'choose', 'unique', 'all')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _selector(cor, n_cells):
    """n_cells x N 0/1 matrix, rows ascending within a cell: S @ A adds every column in ascending row order from 0 (csr_matmat),
    exactly like A[rows].sum(0), and keeps the non-zero sums only."""
    keep = np.flatnonzero(cor >= 0)
    return sp.csr_matrix((np.ones(len(keep)), (cor[keep], keep)), shape=(n_cells, len(cor)))


def _want(tl, method, cor, n_cells, initial, seed):
    np.random.seed(seed)
    mat = tl.reassign(method, 0.9, initial).tocsr()
    return mat, (_selector(cor, n_cells) @ mat.astype(np.float64)).tocsr()


def _got(tl, method, cor, n_cells, initial, seed):
    np.random.seed(seed)
    return tl.reassign_cell_counts(method, cor, n_cells, 0.9, initial)


def _check_csr(got, n_cells, k):
    assert got.shape == (n_cells, k) and got.dtype == np.float64
    assert got.has_sorted_indices or got.nnz == 0
    for c in range(n_cells):                             # columns strictly ascending, only non-zero sums stored
        cols = got.indices[got.indptr[c]:got.indptr[c + 1]]
        assert np.all(np.diff(cols) > 0)
    assert np.all(got.data != 0)


def _same(got, want):
    """bit-identical: same pattern, same values"""
    want = want.tocsr(); want.sort_indices()
    return (np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices)
            and np.array_equal(got.data.view(np.uint64), want.data.view(np.uint64)))


def _run_case(name, options=None):
    import logging
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case(name)
    raw = case_matrix(c)
    tl = TelescopeLikelihood(raw, Opts(c), engine_options=options)
    tl.em(use_likelihood=bool(c['use_likelihood']), loglev=logging.DEBUG)
    return c, raw, tl


def _cells(rng, n, n_cells, none_frac=0.1):
    cor = rng.randint(0, n_cells, n).astype(np.int32)
    cor[rng.rand(n) < none_frac] = -1
    return cor


@pytest.mark.parametrize('name', case_names())
def test_cell_counts_equal_scipy_sum_of_the_device_matrix(gpu_device, name):
    from oracle.telescope_oracle import OracleModel
    c, raw, tl = _run_case(name)
    rng = np.random.RandomState(11)
    n_cells = max(1, min(60, tl.N // 3))
    cor = _cells(rng, tl.N, n_cells)
    om = OracleModel(raw, float(c['pi_prior']), float(c['theta_prior']))
    om.em(float(c['em_epsilon']), int(c['max_iter']), use_likelihood=bool(c['use_likelihood']))
    S = _selector(cor, n_cells)
    for initial in (False, True):
        for method in ALL_METHODS:
            got = _got(tl, method, cor, n_cells, initial, 7)
            _check_csr(got, n_cells, tl.K)
            _, want = _want(tl, method, cor, n_cells, initial, 7)
            assert _same(got, want), (name, method, initial)
            for cell in (0, n_cells - 1):                # the issue's literal form: reassign(...)[rows].sum(0)
                np.random.seed(7)
                rows = np.flatnonzero(cor == cell)
                lit = np.asarray(tl.reassign(method, 0.9, initial).tocsr()[rows].sum(0)).ravel()
                assert np.array_equal(got[cell].toarray().ravel(), lit.astype(np.float64)), (name, method, cell)
            np.random.seed(7)
            owant = (S @ sp.csr_matrix(om.reassign(method, 0.9, initial)).astype(np.float64)).toarray()
            if method in INT_METHODS:
                assert np.array_equal(got.toarray(), owant), (name, method, initial)
            else:
                assert np.allclose(got.toarray(), owant, rtol=RTOL, atol=1e-12), (name, method, initial)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_matrices_and_partitions(gpu_device, seed):
    from telescope_amd.likelihood import TelescopeLikelihood
    rng = np.random.RandomState(seed)
    n, k = int(rng.randint(2000, 9000)), int(rng.randint(30, 3000))
    lens = rng.randint(1, min(k, 40), n)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    raw = sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), indices, indptr), shape=(n, k))
    tl = TelescopeLikelihood(raw, Opts(max_iter=30))
    tl.em()
    n_cells = int(rng.randint(1, 500))
    cor = _cells(rng, n, n_cells, none_frac=rng.rand() * 0.5)
    for method in ALL_METHODS:
        got = _got(tl, method, cor, n_cells, False, seed)
        _check_csr(got, n_cells, k)
        assert _same(got, _want(tl, method, cor, n_cells, False, seed)[1]), method


def _plain_tl(raw, options=None, iters=20):
    from telescope_amd.likelihood import TelescopeLikelihood
    tl = TelescopeLikelihood(raw, Opts(max_iter=iters), engine_options=options)
    tl.em()
    return tl


def _rand_raw(rng, n, k, max_len, wide_rows=0):
    lens = rng.randint(1, max_len, n)
    lens[:wide_rows] = k
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.arange(k) if l == k else np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    return sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), indices, indptr), shape=(n, k))


def test_edge_partitions(gpu_device):
    rng = np.random.RandomState(5)
    # a group with 20k distinct columns: 3000 rows of up to 30 entries over 20000 loci
    k = 20000
    raw = _rand_raw(rng, 3000, k, 30, wide_rows=2)
    tl = _plain_tl(raw)
    n = tl.N
    cases = {
        'one_wide_group': np.zeros(n, np.int32),                       # every row: equals the column sums of tsem_reassign
        'singletons_empty_none': np.where(np.arange(n) % 3 == 0, -1, np.arange(n)).astype(np.int32),
        'contiguous': (np.arange(n) * 7 // n).astype(np.int32),
        'scattered': (np.arange(n) * 7919 % 13).astype(np.int32),
        'largest_last': np.where(np.arange(n) < n // 4, np.arange(n) % 50, 50).astype(np.int32),
    }
    ncells = {'one_wide_group': 1, 'singletons_empty_none': n + 2, 'contiguous': 7, 'scattered': 13, 'largest_last': 51}
    for label, cor in cases.items():
        for method in ALL_METHODS:
            got = _got(tl, method, cor, ncells[label], False, 3)
            _check_csr(got, ncells[label], k)
            assert _same(got, _want(tl, method, cor, ncells[label], False, 3)[1]), (label, method)
            if label == 'one_wide_group':
                np.random.seed(3)
                cs = tl.reassign_colsums(method, 0.9)
                if method in INT_METHODS:
                    assert np.array_equal(got.toarray().ravel(), cs), method
                else:
                    assert np.allclose(got.toarray().ravel(), cs, rtol=1e-12, atol=0), method
    got = tl.reassign_cell_counts('exclude', np.full(n, -1, np.int32), 0)   # n_groups = 0
    assert got.shape == (0, k) and got.nnz == 0
    got = tl.reassign_cell_counts('all', np.full(n, -1, np.int32), 4)       # no row in any cell
    assert got.shape == (4, k) and got.nnz == 0 and np.array_equal(got.indptr, np.zeros(5))


def test_largest_group_ends_at_the_last_entry_with_small_tiles(gpu_device):
    """The last group holds the matrix's last entry; tiles of a few KB cut it into pieces of rows (running totals carried between
    pieces) and pack the other groups several to a tile."""
    rng = np.random.RandomState(8)
    raw = _rand_raw(rng, 6000, 700, 25)
    n = raw.shape[0]
    cor = np.where(np.arange(n) < 2000, np.arange(n) % 300, 300).astype(np.int32)
    for tile in (1 << 16, 1 << 20, 0):
        tl = _plain_tl(raw, options={'group_tile_bytes': tile})
        for method in ALL_METHODS:
            got = _got(tl, method, cor, 301, False, 4)
            assert _same(got, _want(tl, method, cor, 301, False, 4)[1]), (tile, method)


@pytest.mark.parametrize('options', [
    {'value_format': 2}, {'value_format': 1}, {'split': 1, 'parts': 6}, {'drop_csr_indices': 1}, {'reproducible': 1}])
def test_layouts(gpu_device, options):
    rng = np.random.RandomState(21)
    raw = _rand_raw(rng, 5000, 1200, 30)
    ref = _plain_tl(raw)
    tl = _plain_tl(raw, options=options)
    n = tl.N
    n_cells = 40
    cor = _cells(rng, n, n_cells)
    groups = [np.flatnonzero(cor == g) for g in range(n_cells)]
    for method in ALL_METHODS:
        a = _got(tl, method, cor, n_cells, False, 9)
        b = _got(tl, method, cor, n_cells, False, 9)
        assert _same(a, b), (options, method)                       # identical across two calls
        assert _same(a, _want(tl, method, cor, n_cells, False, 9)[1]), (options, method)
        np.random.seed(9)
        dense = tl.reassign_group_sums(method, groups, 0.9)
        if method in INT_METHODS:
            assert np.array_equal(a.toarray(), dense), (options, method)
            assert _same(a, _want(ref, method, cor, n_cells, False, 9)[1]), (options, method)
        else:
            assert np.allclose(a.toarray(), dense, rtol=1e-12, atol=1e-12), (options, method)


def test_droplet_scale(gpu_device):
    """20M rows x 30k loci x ~8 entries: 10k cells of lognormal sizes plus 200k barcodes of 1-3 fragments.  Every method completes
    within the 1 GB scratch bound; the sum over cells equals the column sums over the rows that have a cell."""
    from telescope_amd import _lib, synthetic
    from telescope_amd.likelihood import TelescopeLikelihood
    rng = np.random.RandomState(2026)
    n, k = 20_000_000, 30_000
    eng = _lib.Engine(0)
    eng.generate(0, n, k, synthetic.poisson_cdf_u32(8), 7, synthetic.DIST_CODE['zipf'], 0.0)
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=5, em_epsilon=0.0))
    tl.em()
    assert (tl.N, tl.K) == (n, k) and tl._eng.dims()[2] > 7 * n
    big = np.maximum(1, rng.lognormal(5.5, 1.0, 10_000)).astype(np.int64)
    small = rng.randint(1, 4, 200_000)
    sizes = np.concatenate([big, small])
    sizes = sizes[np.cumsum(sizes) <= n * 0.9] if sizes.sum() > n * 0.9 else sizes
    cor = np.full(n, -1, np.int32)
    perm = rng.permutation(n)[:int(sizes.sum())]
    cor[perm] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    n_cells = len(sizes)
    has = np.flatnonzero(cor >= 0).astype(np.int32)
    for method in ALL_METHODS:
        np.random.seed(1)
        got = tl.reassign_cell_counts(method, cor, n_cells)
        assert got.shape == (n_cells, k)
        if method == 'all':                                  # every row has a hit: every cell has a stored entry
            assert np.all(np.diff(got.indptr) > 0)
        np.random.seed(1)
        picks = tl._dense_picks(tl._picks(tl._which(False))) if method == 'choose' else None
        cs = tl._eng.reassign_rows(method, 0.9, tl._which(False), has, None if picks is None else picks[has])
        tot = np.asarray(got.sum(0)).ravel()
        if method in INT_METHODS:
            assert np.array_equal(tot, cs), method
        else:
            assert np.allclose(tot, cs, rtol=1e-9, atol=1e-9), method


def _sc_run(argv, outdir):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=root,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def _check_reference_files(outdir):
    tag = os.path.join(str(outdir), 'telescope-')
    assert open(tag + 'run_stats.tsv').read() == open(os.path.join(GOLDEN, 'sc_ref-run_stats.tsv')).read()
    for method in ('all', 'unique', 'exclude', 'choose'):
        assert open(tag + 'TE_counts_%s.tsv' % method).read() == open(os.path.join(GOLDEN, 'sc_ref-TE_counts_%s.tsv' % method)).read(), method
    import pandas as pd
    for method in ('conf', 'average'):
        got = pd.read_csv(tag + 'TE_counts_%s.tsv' % method, sep='\t', index_col=0)
        want = pd.read_csv(os.path.join(GOLDEN, 'sc_ref-TE_counts_%s.tsv' % method), sep='\t', index_col=0)
        assert list(got.index) == list(want.index) and list(got.columns) == list(want.columns)
        assert np.allclose(got.values, want.values, rtol=1e-12, atol=0), method


def test_sc_assign_and_resume_reproduce_the_reference_files(gpu_device, tmp_path):
    bam, gtf = os.path.join(GOLDEN, 'sc_mixed.bam'), os.path.join(GOLDEN, 'sc_mixed.gtf')
    _sc_run(['sc', 'assign', bam, gtf, '--use_every_reassign_mode'], tmp_path / 'a')
    _check_reference_files(tmp_path / 'a')
    _sc_run(['sc', 'resume', str(tmp_path / 'a' / 'telescope-checkpoint.npz'), '--use_every_reassign_mode'], tmp_path / 'r')
    _check_reference_files(tmp_path / 'r')
    _sc_run(['sc', 'resume', str(tmp_path / 'a' / 'telescope-checkpoint.npz'), '--count_format', 'mtx'], tmp_path / 'm')
    import scipy.io
    import pandas as pd
    m = scipy.io.mmread(str(tmp_path / 'm' / 'telescope-TE_counts.mtx')).toarray()
    want = pd.read_csv(os.path.join(GOLDEN, 'sc_ref-TE_counts_exclude.tsv'), sep='\t', index_col=0)
    assert np.array_equal(m, want.values)
    assert open(str(tmp_path / 'm' / 'telescope-barcodes.tsv')).read().split() == list(want.index)
