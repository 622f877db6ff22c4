"""Cases for the SPREAD class of the per-group EM fits (engine option "cell_em_spread_entries", tsem_cellem.hip): groups at the edges
of its column tiers and row chunks, and the cell-type partition of the end-to-end fixture.  The yardstick stays the oracle run per
group (tests/_cell_em_reference.py: CellRef, RTOL = 1e-9, iteration counts equal); every reference is computed once per session.
Shared by tests/test_gpu_group_em.py and tests/test_celltype_host.py."""
import functools
import os

import numpy as np

import _cell_em_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# The constants of the spread class as include/telescope_em.h documents them (tsem_cell_em): threads of a workgroup = columns per
# batch, rows per chunk, the largest column one lane adds, the largest a wave adds, iterations enqueued per look of the host.
SP_T, SP_ROWS, SP_LANE, SP_WAVE, SP_LOOK = 256, 1024, 32, 4096, 8

# (Kc, entries) per group: boundary_matrix lays the entries cyclically over the Kc columns, so (4, 4 n + 2) gives two columns of n
# and two of n + 1 entries, (2, 2 n + 1) one of n and one of n + 1.
TIER_K = 64
TIER_GROUPS = (
    (4, 4 * SP_LANE + 2),                                  # L | L + 1: one lane | a wave
    (4, 4 * 64 + 2),                                       # 64 | 65: the wave tier at one entry per lane | the first piece of two
    (4, 4 * 64 * 3 + 2),                                   # 64 m | 64 m + 1 at m = 3
    (2, 2 * SP_WAVE + 1),                                  # 4096 | 4097: a wave | the workgroup
    (2, 2 * SP_T * 17 + 1),                                # 256 m | 256 m + 1 at m = 17
    (3, 5),                                                # (two entries per column at most)
)
TIER_PARAMS = R.B_PARAMS                                   # (pi_prior, theta_prior, use_likelihood)


@functools.lru_cache(maxsize=None)
def tier_case():
    raw, cor, cols = R.boundary_matrix(33, TIER_K, TIER_GROUPS)
    return raw, cor, len(TIER_GROUPS)


def column_counts(raw, cor, c):
    """entries per touched column of group c, ascending"""
    sub = raw[np.flatnonzero(np.asarray(cor) == c)].tocsc()
    n = np.diff(sub.indptr)
    return sorted(n[n > 0].tolist())


@functools.lru_cache(maxsize=None)
def chunk_case():
    """Groups of exactly one chunk of rows, one chunk + 1 and one row (with two entries at least, so that it is spread when forced),
    cut from one random matrix in row order; the other rows are in no group."""
    raw, _ = R.random_matrix(41, 2 * SP_ROWS + 400, 50, 1)
    lens = np.diff(raw.indptr)
    cor = np.full(raw.shape[0], -1, np.int32)
    cor[:SP_ROWS] = 0
    cor[SP_ROWS:2 * SP_ROWS + 1] = 1
    rest = np.arange(2 * SP_ROWS + 1, raw.shape[0])
    cor[rest[lens[rest] > 1][0]] = 2
    return raw, cor, 3


@functools.lru_cache(maxsize=None)
def twin_case():
    return R.twin_tie_matrix(n_cells=2)


def _shape(seed):
    return lambda: R.shape_case(seed)[:3]


NAMED = dict(R.NAMED)
NAMED.update({'tiers': tier_case, 'chunks': chunk_case, 'twins2': twin_case, 'shape3': _shape(3), 'shape4': _shape(4), 'shape5': _shape(5)})


@functools.lru_cache(maxsize=None)
def group_ref(key, pi_prior, theta_prior, use_likelihood=False, max_iter=R.MAX_ITER):
    """The oracle's fits of a named matrix, once per session (the cases of tests/_cell_em_reference.py through its own cache)."""
    if key in R.NAMED:
        return R.cell_ref(key, pi_prior, theta_prior, use_likelihood, max_iter)
    raw, cor, n = NAMED[key]()
    return R.CellRef(raw, cor, n, pi_prior, theta_prior, max_iter=max_iter, use_likelihood=use_likelihood)


def shape_ref(seed):
    """the existing reference of a random shape (SHAPES' own priors and stop test)"""
    return R.shape_case(seed)[3]


# ---- the cases the GPU tests compare iteration counts on: (label, reference) — tests/test_celltype_host.py asserts that no stop
# test of any of them lies within 1e-6 relative of epsilon (the spread class rounds differently from the other classes) ----
LOOK_ITERS = (1, SP_LOOK - 1, SP_LOOK, SP_LOOK + 1)        # max_iter around the host's look interval
DEGENERATE_PRIORS = ((0, 200000), (1, 5), (0, 0))


def iteration_count_cases():
    for seed in (1, 3, 4, 5):
        yield 'shape %d' % seed, shape_ref(seed)
    for params in TIER_PARAMS:
        yield 'tiers %s' % (params,), group_ref('tiers', *params)
        yield 'B %s' % (params,), group_ref('B', *params)
    yield 'chunks', group_ref('chunks', 0, 200000)
    yield 'twins', group_ref('twins2', 0, 200000)
    for m in LOOK_ITERS:
        yield 'tiers, max_iter %d' % m, group_ref('tiers', 0, 200000, False, m)
        yield 'shape 3, max_iter %d' % m, group_ref('shape3', 0, 0, False, m)
    for priors in DEGENERATE_PRIORS:
        for key in ('empty_rows', 'full_columns', 'K2', 'K1'):
            yield '%s %s' % (key, priors), group_ref(key, *priors)
    yield 'two maps', two_maps_case()[3]
    yield 'two maps, twin ties', two_maps_twin_case()[3]
    yield 'end to end', e2e_case()[3]


# ---- a fit under a type map, counts under the barcode map ----
def _types_of(cor, n_cells, per_type, drop):
    """cells -> types of `per_type` consecutive cells; the cells in `drop` have no type"""
    toc = (np.arange(n_cells) // per_type).astype(np.int32)
    toc[list(drop)] = -1
    tor = np.where(cor >= 0, toc[np.maximum(cor, 0)], -1).astype(np.int32)
    return toc, tor, int(toc.max()) + 1


@functools.lru_cache(maxsize=None)
def two_maps_case():
    """shape 1: 40 barcodes in 5 types of 8, barcodes 3 and 17 in none.  (raw, barcode of row, type of row, reference, n_types)"""
    raw, cor, n_cells, _ = R.shape_case(1)
    toc, tor, n_types = _types_of(cor, n_cells, 8, (3, 17))
    return raw, cor, tor, R.CellRef(raw, tor, n_types, 0, 200000), n_types


@functools.lru_cache(maxsize=None)
def two_maps_twin_case():
    """the twin-tie matrix (every tie a twin tie: both sides draw `choose` for the same rows): 20 barcodes in 4 types of 5"""
    raw, cor, n_cells = R.twin_tie_matrix()
    toc, tor, n_types = _types_of(cor, n_cells, 5, (6,))
    return raw, cor, tor, R.CellRef(raw, tor, n_types, 0, 200000), n_types


# ---- end to end: tests/golden/sc_mixed.bam with tests/golden/sc_mixed_celltypes.tsv ----
E2E_TSV = os.path.join(GOLDEN, 'sc_mixed_celltypes.tsv')
E2E_TYPES = ('Bcell', 'Tcell')
E2E_OMITTED = 'ACGT'


def load_sc_mixed():
    """the fixture's run container from the BAM, on the host (no device)"""
    from telescope_amd.loader import Annotation
    from telescope_amd.run_container import scTelescope

    class O(object):
        samfile = os.path.join(GOLDEN, 'sc_mixed.bam')
        no_feature_key, overlap_mode, overlap_threshold, stranded_mode, barcode_tag, updated_sam = '__no_feature', 'threshold', 0.2, 'None', 'CB', False
    ts = scTelescope(O())
    ts.load_alignment(Annotation(os.path.join(GOLDEN, 'sc_mixed.gtf'), 'locus', 'None'))
    return ts


def e2e_reference(ts):
    """(type of row, reference) of a loaded sc_mixed run under the fixture's cell types"""
    import scipy.sparse as sp
    from telescope_amd.run_container import celltype_map, compose_type_of_row, read_celltype_tsv
    names, toc = celltype_map(ts.barcodes, read_celltype_tsv(E2E_TSV))
    assert tuple(names) == E2E_TYPES
    tor = compose_type_of_row(ts.cell_of_row, toc)
    return tor, R.CellRef(sp.csr_matrix(ts.raw_scores), tor, len(names), 0, 200000)


@functools.lru_cache(maxsize=None)
def e2e_case():
    ts = load_sc_mixed()
    tor, ref = e2e_reference(ts)
    return ts, np.asarray(ts.cell_of_row), tor, ref
