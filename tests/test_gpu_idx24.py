"""The 3-byte entry index of the fused layouts with fp64 entries (telescope_amd/csrc/tsem_idx24.h): 11 instead of 12 bytes per stored
entry in the stream of the fused EM / lnl passes.  Where it is in use, that it decodes to the layout the 32-bit index holds, what the
accounting says, parity with the oracle over the team sizes and geometries, and the layouts that must keep the 32-bit index."""
import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
from test_gpu_parity import RTOL, _oracle_vs_gpu, _synthetic_tl

pytestmark = pytest.mark.gpu

_MATS = {}


def _zipf(cols, rows=60000, d=24):
    """synthetic 60 000 x cols, ~24 entries per row, 5 % unique rows (generated once per shape)."""
    from telescope_amd import synthetic
    if (rows, cols, d) not in _MATS:
        ip, ix, rw = synthetic.generate(rows, cols, d, seed=11, dist='zipf', uniq_frac=0.05)
        _MATS[(rows, cols, d)] = sp.csr_matrix((rw, ix, ip), shape=(rows, cols))
    return _MATS[(rows, cols, d)]


def _short_rows():
    """The matrix of test_short_row_geometry_with_any_block_size: 2..6 entries per row, geometry 3, up to 1152 row slots."""
    if 'short' not in _MATS:
        rng = np.random.RandomState(77)
        n, k = 30000, 16000
        lens = rng.randint(2, 7, n)
        indptr = np.concatenate([[0], np.cumsum(lens)])
        indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
        data = rng.randint(139, 213, indptr[-1]).astype(np.uint16)
        _MATS['short'] = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    return _MATS['short']


def _load(raw, options):
    """An engine with the layout built (no EM)."""
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    eng = _lib.Engine(0)
    for k, v in options:
        eng.set_option(k, v)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=2, em_epsilon=0.0))
    return tl, eng


def test_packed_index_decodes_to_the_layout_of_the_32_bit_index(gpu_device):
    """The same fill kernel on the same input, once storing the 3-byte index (fp64 entries) and once the 32-bit one (score codes, entry
    order left alone): same block boundaries, and every sub-block holds the same (row slot, column slot) pairs.  Kp ~ 7500: column bit
    12 is in use, the hot column is dealt over several slots."""
    raw = _zipf(30000)
    _, probe = _load(raw, (('value_format', 1),))
    shape = probe.layout_info()
    del probe
    forced = (('block_rows', shape['R']), ('geometry', shape['geometry']))
    tl_a, a = _load(raw, (('value_format', 1),) + forced)
    tl_b, b = _load(raw, (('value_format', 2), ('deconflict', 0)) + forced)
    ia, ib = a.layout_info(), b.layout_info()
    assert ia['fused'] == 1 and ib['fused'] == 1 and ia['row_order'] == 1 and ib['row_order'] == 1
    assert ia['P'] == 4 and ia['Kp'] > 4096
    assert [ia[k] for k in ('P', 'Kp', 'R', 'nb', 'nnz_pad')] == [ib[k] for k in ('P', 'Kp', 'R', 'nb', 'nnz_pad')]
    assert ia['index_bytes'] == 3 and ia['value_bytes'] == 8
    assert ib['index_bytes'] == 4 and ib['value_bytes'] == 2
    seen_hi_col = False
    for blk in range(min(20, ia['nb'])):
        for part in range(ia['P']):
            wa, wb = a.debug_subblock(blk, part), b.debug_subblock(blk, part)
            assert wa.size == wb.size and wa.size % 64 == 0
            assert np.array_equal(np.sort(wa), np.sort(wb)), (blk, part)
            assert int((wa >> 16).max()) < ia['R'] and int((wa & 0xFFFF).max()) < ia['Kp']
            assert np.all(np.diff((wa >> 16).astype(np.int64)) >= 0), (blk, part)    # row order survives the decoding
            seen_hi_col |= bool(((wa & 0xFFFF) >= 4096).any())
    assert seen_hi_col
    # bytes as stored: what bench.py takes its roofline from, and what a capacity plan counts
    for eng, info, per_entry in ((a, ia, 11), (b, ib, 6)):
        assert eng.kernel_stats()['algo_bytes_per_pass'] == per_entry * info['nnz_amb'] + 2 * info['N_amb']
    la, lb = a.device_memory()['resident']['layout'], b.device_memory()['resident']['layout']
    assert la - lb == (3 + 8 - 4 - 2) * ia['nnz_pad']


def test_layout_bytes_fall_by_one_byte_per_padded_entry(gpu_device):
    """fp64 entries behind the 3-byte index (fused kernel) and behind the 32-bit index (two-pass kernels): the layout's resident bytes
    are (index + 8) per padded entry plus 12 per sub-block offset — one byte per padded entry less at the same padded size."""
    raw = _zipf(5000)
    _, a = _load(raw, (('value_format', 1),))
    ia = a.layout_info()
    _, b = _load(raw, (('value_format', 1), ('em_kernel', 1), ('block_rows', ia['R'])))
    ib = b.layout_info()
    assert ia['index_bytes'] == 3 and ia['fused'] == 1 and ib['index_bytes'] == 4 and ib['fused'] == 0
    for eng, info in ((a, ia), (b, ib)):
        assert eng.device_memory()['resident']['layout'] == \
            (info['index_bytes'] + 8) * info['nnz_pad'] + 12 * (info['nb'] * info['P'] + 2)
    assert b.kernel_stats()['algo_bytes_per_pass'] == 12 * ib['nnz_amb'] + 2 * ib['N_amb']


@pytest.mark.parametrize('cols,parts', [(5000, 1), (30000, 4), (60000, 8)])
def test_packed_index_against_the_oracle(gpu_device, cols, parts):
    """fp64 entries on the fused kernel — EM passes and lnl passes read the 3-byte index — with no exchange (P = 1), teams of 4 and
    teams of 8 (three exchange waves)."""
    info = _oracle_vs_gpu(_zipf(cols), iters=4, options=(('value_format', 1),))
    assert info['P'] == parts and info['fused'] == 1 and info['split'] == 0
    assert info['index_bytes'] == 3 and info['value_bytes'] == 8


@pytest.mark.parametrize('block_rows', [1152, 200])
def test_packed_index_with_short_rows(gpu_device, block_rows):
    """Geometry 3 with 1152 row slots (row bit 10 is set) and with a block size far below what the exchange waves cover."""
    info = _oracle_vs_gpu(_short_rows(), iters=4, options=(('value_format', 1), ('block_rows', block_rows)))
    assert info['fused'] == 1 and info['geometry'] == 3 and info['R'] == block_rows
    assert info['index_bytes'] == 3


def test_split_and_two_pass_layouts_keep_the_32_bit_index(gpu_device):
    """Parts of more than 8192 columns (split layout) and the two-pass kernels read lrow << 16 | lcol as before."""
    from telescope_amd import synthetic
    ip, ix, rw = synthetic.generate(30000, 70000, 30, seed=17, dist='zipf', uniq_frac=0.05)
    info = _oracle_vs_gpu(sp.csr_matrix((rw, ix, ip), shape=(30000, 70000)), iters=4, options=(('value_format', 1),))
    assert info['fused'] == 1 and info['split'] == 1 and info['index_bytes'] == 4
    info = _oracle_vs_gpu(_zipf(30000), iters=4, options=(('value_format', 1), ('em_kernel', 1)))
    assert info['fused'] == 0 and info['index_bytes'] == 4 and info['value_bytes'] == 8


def test_fall_back_from_a_packed_layout_rebuilds_the_32_bit_index(gpu_device):
    """fused_dbg = 32: the first EM pass reports a hand-off time-out.  The handle rebuilds its layout for the two-pass kernels — with
    the 32-bit index they read — redoes the step and ends where the oracle ends."""
    info = _oracle_vs_gpu(_zipf(30000), iters=4, options=(('value_format', 1), ('fused_dbg', 32)))
    assert info['fused'] == 0 and info['index_bytes'] == 4 and info['fallbacks'] == 1


def test_reproducible_mode_with_fp64_entries(gpu_device):
    """`reproducible` with fp64 entries (MODE 2 of the fused kernel reads the 3-byte index): two engines agree bit for bit, and with
    the C oracle to the usual tolerance."""
    from oracle import em_fused as oc
    runs = []
    for rep in range(2):
        tl = _synthetic_tl(300_000, 15_000, 40, 'zipf', uniq=0.05, options=(('value_format', 1), ('reproducible', 1)),
                           opts=Opts(max_iter=5, em_epsilon=0.0))
        info = tl._eng.layout_info()
        assert info['reproducible'] == 1 and info['fused'] == 1 and info['index_bytes'] == 3
        tl.em()
        runs.append((tl.n_iter, tl.pi.copy(), tl.theta.copy(), tl.lnl))
        if rep == 0:
            ip, ix, rw = tl._eng.export_csr()
            ref = oc.em_fused_arrays(ip, ix, rw, 15_000, 0, 200000, 0.0, 5)
        del tl
    a, b = runs
    assert a[0] == b[0] == ref['n_iter'] == 5
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]
    assert abs(a[3] - ref['lnl']) <= RTOL * abs(ref['lnl'])
    assert np.allclose(a[1], ref['pi'], rtol=RTOL, atol=0) and np.allclose(a[2], ref['theta'], rtol=RTOL, atol=0)
