"""Option `drop_csr_indices`: the CSR column ids (4 B per stored entry) are rebuilt for every call that reads them and are gone again
when the call returns — on its error paths too — while the calls that never read them leave the matrix alone.  Two engines over one
matrix, `drop_csr_indices` 0 and 1; after the pooled fit both get the SAME parameters (the first engine's, set twice so that the
previous and the current ones agree), so every row pass reads the same numbers: what the row passes decide per row or per entry is
compared as bits, what they add up with floating-point atomics to the tolerances of tests/test_gpu_round5.py.

The matrix: 2000 rows x 300 columns, ~8 entries per row, a tenth of the rows with one entry; 20 groups, one of them empty, one large
enough to be cut across the tiles of the sparse per-group counts, some rows in no group."""
import ctypes as C

import numpy as np
import pytest

from conftest import Opts

pytestmark = pytest.mark.gpu
METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')
INTEGER = ('exclude', 'choose', 'unique', 'all')            # masks of 0 / 1: their sums are exact
N_ROWS, N_COLS, N_GROUPS, EMPTY_GROUP, BIG_GROUP = 2000, 300, 20, 7, 3


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _ids(tl):
    return tl._eng.device_memory()['resident']['csr_indices']


def _group_map():
    """row -> group: group 3 holds the first 500 rows (cut across tiles), group 7 none, every 11th row of the rest belongs to no group"""
    g = np.empty(N_ROWS, np.int32)
    g[:500] = BIG_GROUP
    others = [x for x in range(N_GROUPS) if x not in (BIG_GROUP, EMPTY_GROUP)]
    g[500:] = np.asarray(others, np.int32)[np.arange(N_ROWS - 500) % len(others)]
    g[500::11] = -1
    return g


@pytest.fixture(scope='module')
def pair(gpu_device):
    """(keep, drop, raw, group map): the two fitted objects on the same parameters"""
    from telescope_amd import synthetic
    from telescope_amd.likelihood import TelescopeLikelihood
    raw = synthetic.generate_csr(N_ROWS, N_COLS, 8.0, seed=11, dist='zipf', uniq_frac=0.1)
    assert (np.diff(raw.indptr) == 1).sum() > 50
    tls = []
    for drop in (0, 1):
        tl = TelescopeLikelihood(raw, Opts(max_iter=6, em_epsilon=0.0), device=gpu_device, engine_options={'drop_csr_indices': drop})
        tl.em()
        tls.append(tl)
    keep, dropping = tls
    assert _ids(keep) >= 4 * raw.nnz and _ids(dropping) == 0
    pi, theta = keep._eng.get_params()
    for tl in tls:
        tl._eng.set_params(pi, theta)
        tl._eng.set_params(pi, theta)                             # previous = current = the first engine's
        tl.pi, tl.theta = pi.copy(), theta.copy()
    return keep, dropping, raw, _group_map()


def _both(pair, call, same, label):
    """`call(tl)` on both objects from the same RNG state; the ids are gone again after the dropping one's; `same(a, b)` holds"""
    keep, dropping = pair[0], pair[1]
    out = []
    for tl in (keep, dropping):
        np.random.seed(5)
        out.append(call(tl))
        if tl is dropping:
            assert _ids(tl) == 0, '%s left the CSR column ids resident' % label
    assert same(out[0], out[1]), label
    return out[0]


def _close(a, b):
    return np.allclose(a, b, rtol=1e-10, atol=1e-10)


def test_z_and_the_explicit_steps(pair):
    from telescope_amd._lib import Z_PREV
    keep = pair[0]
    z = _both(pair, lambda tl: tl._eng.export_z(Z_PREV), _same_bits, 'export_z')
    zs = _both(pair, lambda tl: tl.estep(tl.pi, tl.theta).data, _same_bits, 'estep')
    zm = keep.estep(keep.pi, keep.theta)
    _both(pair, lambda tl: np.concatenate(tl.mstep(zm)), lambda a, b: np.allclose(a, b, rtol=1e-11, atol=0), 'mstep')
    _both(pair, lambda tl: tl.calculate_lnl(zm, tl.pi, tl.theta), lambda a, b: abs(a - b) <= 1e-12 * abs(a), 'calc_lnl')
    assert z.size == pair[2].nnz and zs.size > 0


def test_best_hits_and_ties(pair):
    from telescope_amd._lib import Z_INITIAL, Z_PREV
    for which in (Z_INITIAL, Z_PREV):
        _both(pair, lambda tl: tl._eng.best_counts(which), np.array_equal, 'best_counts')
        _both(pair, lambda tl: np.concatenate(tl._eng.best_ties(which)), np.array_equal, 'best_ties')


def test_an_error_after_the_rebuild_drops_the_ids_again(pair):
    """tsem_best_ties with arrays shorter than the tie count: it finds that out after its row pass, returns TSEM_ERR_ARG and the count"""
    from telescope_amd import _lib
    dropping = pair[1]
    eng = dropping._eng
    assert len(eng.best_ties(_lib.Z_INITIAL)[0]) > 1            # equal scores: the initial z has tied rows
    rows, counts, n = np.empty(1, np.int32), np.empty(1, np.int32), C.c_int64()
    rc = eng._L.tsem_best_ties(eng._h, _lib.Z_INITIAL, 1, _lib.ptr(rows), _lib.ptr(counts), C.byref(n))
    assert rc == _lib.ERR_ARG and n.value > 1
    assert _ids(dropping) == 0


@pytest.mark.parametrize('initial', [True, False])
def test_column_sums_of_every_method(pair, initial):
    for tl in pair[:2]:
        tl._report_cache = {}
    for method in METHODS:
        _both(pair, lambda tl: tl.reassign_colsums(method, initial=initial), np.array_equal if method in INTEGER else _close,
              (method, initial))


def test_generic_report_pass(pair):
    """engine option report_kernel = 0: conf | exclude | average and the tie list from k_rowpass<RP_REPORT>"""
    keep, dropping = pair[0], pair[1]
    for tl in (keep, dropping):
        tl._eng.set_option('report_kernel', 0)
        tl._report_cache = {}
    try:
        for initial in (True, False):
            for method in ('exclude', 'average', 'conf', 'choose'):
                _both(pair, lambda tl: tl.reassign_colsums(method, initial=initial), np.array_equal if method in INTEGER else _close,
                      ('report_kernel 0', method, initial))
        assert dropping._eng.report_stats()['kernel'] == 'k_rowpass'
    finally:
        for tl in (keep, dropping):
            tl._eng.set_option('report_kernel', 1)
            tl._report_cache = {}


def test_assignment_matrix(pair):
    for method in ('exclude', 'choose', 'average'):
        m = _both(pair, lambda tl: tl.reassign(method).tocsr(),
                  lambda a, b: np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and _same_bits(a.data, b.data),
                  ('reassign', method))
        assert m.nnz > 0


def test_lookups_and_row_lists(pair):
    from telescope_amd._lib import Z_PREV
    raw = pair[2]
    coo = raw.tocoo()
    sel = np.arange(0, raw.nnz, 7)
    for method in ('exclude', 'choose', 'average'):
        _both(pair, lambda tl: np.concatenate([x.astype(np.float64) for x in tl.lookup(coo.row[sel], coo.col[sel], method)]), _same_bits,
              ('lookup', method))
    rows = np.arange(3, N_ROWS, 5, dtype=np.int32)
    for method in ('exclude', 'all', 'unique'):                 # a list of rows, and (choose, through reassign_colsums) the device's tie list
        _both(pair, lambda tl: tl._eng.reassign_rows(method, 0.9, Z_PREV, rows, None), np.array_equal, ('reassign_rows', method))
    _both(pair, lambda tl: tl._eng.reassign_rows('average', 0.9, Z_PREV, rows, None), _close, ('reassign_rows', 'average'))
    for tl in pair[:2]:
        tl._report_cache = {}
    _both(pair, lambda tl: tl.reassign_colsums('choose'), np.array_equal, 'reassign_rows of the tie list')


def test_dense_group_sums(pair):
    gmap = pair[3]
    groups = [np.flatnonzero(gmap == g) for g in range(N_GROUPS)]
    for method in ('average', 'unique', 'choose'):               # the streaming tiles | k_group_unique | the generic row pass
        out = _both(pair, lambda tl: tl.reassign_group_sums(method, groups), _close if method == 'average' else np.array_equal,
                    ('group sums', method))
        assert not out[EMPTY_GROUP].any() and out[BIG_GROUP].any()


def test_sparse_group_counts_in_tiles(pair):
    """group_tile_bytes = 64 KiB: 682 entries per tile — several tiles, and the 500 rows of group 3 cut into pieces"""
    keep, dropping, raw, gmap = pair
    assert raw[:500].nnz > 3 * ((1 << 16) // 96)
    for tl in (keep, dropping):
        tl._eng.set_option('group_tile_bytes', 1 << 16)
    try:
        for method in METHODS:
            m = _both(pair, lambda tl: tl.reassign_cell_counts(method, gmap, N_GROUPS),
                      lambda a, b: np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and _same_bits(a.data, b.data),
                      ('group_counts', method))
            assert m[EMPTY_GROUP].nnz == 0 and m[BIG_GROUP].nnz > 0
    finally:
        for tl in (keep, dropping):
            tl._eng.set_option('group_tile_bytes', 0)


def test_entry_tag_tiles_keep_the_ids_between_tiles_only(pair):
    keep, dropping, raw, _ = pair
    want = list(keep.entry_tag_tiles('exclude', tile_bytes=16 << 10))
    assert len(want) >= 3
    gen = dropping.entry_tag_tiles('exclude', tile_bytes=16 << 10)
    for i, (r0, r1, words) in enumerate(gen):
        assert (r0, r1) == want[i][:2] and np.array_equal(words, want[i][2])
        assert _ids(dropping) >= 4 * raw.nnz, 'the ids are kept from tile to tile'
    assert i == len(want) - 1 and _ids(dropping) == 0
    gen = dropping.entry_tag_tiles('exclude', tile_bytes=16 << 10)
    next(gen)
    assert _ids(dropping) >= 4 * raw.nnz
    gen.close()                                                    # a caller that stops after the first tile
    assert _ids(dropping) == 0
    _both(pair, lambda tl: tl.entry_tags(10, 900, 'average'), np.array_equal, 'entry_tags')


def test_streaming_passes_leave_a_dropped_matrix_alone(pair):
    dropping, gmap = pair[1], pair[3]
    groups = [np.flatnonzero(gmap == g) for g in range(N_GROUPS)]
    dropping._report_cache = {}
    assert _ids(dropping) == 0
    dropping.reassign_colsums('average')
    assert dropping._eng.report_stats()['kernel'] != 'k_rowpass' and _ids(dropping) == 0
    dropping.reassign_group_sums('exclude', groups)
    assert _ids(dropping) == 0


def test_per_cell_fits(pair):
    """last: afterwards both objects read the per-cell posteriors"""
    from telescope_amd import _lib
    from telescope_amd.likelihood import CellFits
    gmap = pair[3]

    def same(a, b):
        return all(_same_bits(getattr(a[0], f), getattr(b[0], f)) for f in CellFits.FIELDS) and _same_bits(a[1], b[1])
    fits, z = _both(pair, lambda tl: (tl.em_cells(gmap, N_GROUPS), tl._eng.export_z(_lib.Z_USER)), same, 'em_cells')
    assert fits.n_iter[EMPTY_GROUP] == 0 and fits.n_iter[BIG_GROUP] > 0
    for tl in pair[:2]:
        tl.select_z('pooled')
