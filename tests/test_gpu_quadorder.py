"""`-m gpu`: the conflict-aware order inside the quads of the fused layouts with fp64 entries (telescope_amd/csrc/tsem_quadorder.h,
k_quad_order in tsem_setup.hip; option `deconflict` = 1, or auto from `deconflict_min_bytes` on).

  layout      against the layout of the same matrix with `deconflict` = 0, 3-byte and quad index: the same row slot at every position,
              per quad the same (row slot, column slot, value) triples, the device's order equal to tsem_quad_order_host applied to
              the unordered layout's windows, the same sizes, offsets and dummies, the kind and the count in the extended info; teams
              of 1, 2 and 4, a hot column with several slots, sub-blocks of 16, 32, 48 and 0 quads modulo 64, rows of one and two
              entries per part, many dummies;
  passes      one EM pass, one lnl pass and the update against the long-double reference of tests/_em_pass_reference.py with its own
              bounds, on ordered layouts: both index forms, teams of 1, 2 and 4, geometry 2 with the 3-byte index;
  the loop    four iterations with the order on and off (the bars of test_conflict_aware_row_order_option), and how far the worst
              multiplicity falls;
  the choice  the auto rule and its size threshold; `reproducible`, the split layout and the two-pass fall-back keep their order.

Planted mutations (each planted once and seen to fail the tests named; profiles/r30_quad_order.txt section 10):
  the values not moved with their columns — every case of test_layout_against_the_unordered_layout, of
      test_passes_against_the_exact_reference and of test_four_iterations_with_the_order_on_and_off;
  a permutation allowed across a row boundary (ts_qo_same_row always true) — the same, and tests/test_quadorder_host.py (the model
      disagrees, a position changes its row);
  the second value pair addressed with a group width of 64 in a narrower last group — the same GPU tests as the first."""
import numpy as np
import pytest

import _em_pass_reference as E
from conftest import Opts
from test_gpu_em_pass_exact import Model, _leg
from test_gpu_idx24 import _load, _short_rows, _zipf
from test_gpu_parity import _oracle_vs_gpu

pytestmark = pytest.mark.gpu
FP64 = (('value_format', 1),)
IDX = {1: FP64 + (('index_format', 1),), 2: FP64 + (('index_format', 2),)}
ON, OFF = (('deconflict', 1),), (('deconflict', 0),)


def _say(fmt, *a):
    print('QUADORDER ' + fmt % a, flush=True)


def _ext(eng):
    return eng.layout_info(extended=True)


def _sub_blocks(eng, info):
    cap = int(info['nnz_pad']) + 64
    for blk in range(info['nb']):
        for part in range(info['P']):
            w = eng.debug_subblock(blk, part, cap=cap)
            v, rows, cols = eng.debug_subblock_values(blk, part, cap=cap)
            assert len(v) == len(w) and len(w) % 64 == 0 and len(w) < cap
            yield blk, part, w, v, rows, cols


def _worst(words):
    """largest number of lanes per class, for every (window, slot) bin of a sub-block"""
    g = (words & 15).astype(np.int64).reshape(-1, 16, 4)
    return [int(np.bincount(g[x, :, j], minlength=16).max()) for x in range(g.shape[0]) for j in range(4)]


def _sorted_quads(t):
    """[quads x 4 x 3] -> the same with the four triples of every quad in lexicographic order"""
    rec = np.ascontiguousarray(t).view([('w', np.uint64), ('v', np.uint64), ('c', np.uint64)]).reshape(-1, 4)
    return np.sort(rec, axis=1, order=('w', 'v', 'c'))


def _compare(raw, options, label):
    """the ordered layout of `raw` against the unordered one; returns (info, quad counts, worst multiplicity before, after)"""
    from telescope_amd import _lib
    _, a = _load(raw, options + ON)
    _, b = _load(raw, options + OFF)
    ia, ib = _ext(a), _ext(b)
    assert ib['order_kind'] == 0 and ib['order_quads_moved'] == 0, (label, ib)
    assert ia['order_kind'] == 2 and ia['order_quads_moved'] > 0, (label, ia)
    same = ('P', 'Kp', 'R', 'nb', 'N_amb', 'nnz_amb', 'nnz_pad', 'max_subblock', 'index_bytes', 'index_format', 'index_dummies',
            'index_unrepresentable', 'hot_cols', 'geometry', 'fused', 'split', 'row_order', 'lds_bytes')
    assert [ia[k] for k in same] == [ib[k] for k in same], (label, ia, ib)
    assert ia['fused'] == 1 and ia['split'] == 0 and ia['row_order'] == 1 and ia['value_bytes'] == 8, (label, ia)
    assert a.kernel_stats()['algo_bytes_per_pass'] == b.kernel_stats()['algo_bytes_per_pass'], label
    moved, nqs, before, after = 0, [], [], []
    for (blk, part, wa, va, ra, ca), (_, _, wb, vb, rb, cb) in zip(_sub_blocks(a, ia), _sub_blocks(b, ib)):
        assert len(wa) == len(wb), (label, blk, part, 'sub-block sizes')
        nqs.append(len(wb) // 4)
        if len(wb) == 0:
            continue
        assert np.array_equal(wa >> 16, wb >> 16), (label, blk, part, 'a position changed its row slot')
        assert np.array_equal(ra, rb), (label, blk, part)
        codes, m = _lib.quad_order_host(wb)
        perm = np.stack([(codes.astype(np.int64) >> (2 * j)) & 3 for j in range(4)], axis=-1)
        moved += m
        ta = np.stack([wa.astype(np.uint64), va.view(np.uint64), ca.astype(np.int64).view(np.uint64)], axis=-1).reshape(-1, 4, 3)
        tb = np.stack([wb.astype(np.uint64), vb.view(np.uint64), cb.astype(np.int64).view(np.uint64)], axis=-1).reshape(-1, 4, 3)
        assert np.array_equal(_sorted_quads(ta), _sorted_quads(tb)), (label, blk, part, 'a quad holds other (row slot, column slot, value) triples')
        want = np.take_along_axis(tb, perm[:, :, None], axis=1)
        bad = np.flatnonzero((ta != want).any(axis=(1, 2)))
        assert len(bad) == 0, (label, blk, part, 'the device order is not the host order in quads', bad[:5], len(wb) // 4)
        real = vb != 0.0
        assert np.all((wb & 0xFFFF)[~real] == 0) and np.all((wa & 0xFFFF)[va == 0.0] == 0), (label, blk, part, 'padding and dummies')
        before += _worst(wb)
        after += _worst(wa)
    assert moved == ia['order_quads_moved'], (label, moved, ia['order_quads_moved'])
    return ia, np.array(nqs), float(np.mean(before)), float(np.mean(after))


LAYOUT_CASES = {
    'zipf-p4': lambda: [(_zipf(30000), (('block_rows', 512), ('geometry', 0)))],
    'zipf-p2': lambda: [(_zipf(9000), (('block_rows', 512), ('geometry', 0)))],
    'zipf-p1': lambda: [(_zipf(5000), (('block_rows', 512), ('geometry', 0)))],
    'short': lambda: [(_short_rows(), (('block_rows', 512), ('geometry', 0)))],
    # block_rows = 64: sub-blocks of 16, 32, 48 and 0 quads modulo the value map's group of 64, some shorter than a group
    'residues': lambda: [(E.matrix('ring', E.REDUCED['ring']), (('parts', 1), ('block_rows', 64), ('geometry', 0))),
                         (E.matrix('row_shape'), (('parts', 4), ('block_rows', 64), ('geometry', 0)))],
}


@pytest.mark.parametrize('index', [1, 2])
@pytest.mark.parametrize('case', sorted(LAYOUT_CASES))
def test_layout_against_the_unordered_layout(gpu_device, case, index):
    residues, short, whole = set(), 0, 0
    for raw, forced in LAYOUT_CASES[case]():
        info, nqs, m0, m1 = _compare(raw, IDX[index] + forced, (case, index))
        assert info['index_format'] == index and info['index_bytes'] == (3 if index == 1 else 2), info
        nz = nqs[nqs > 0]
        _say('%s index %d: P %d nb %d, quads per sub-block %d .. %d, %d dummies, %d of %d quads moved, worst multiplicity %.3f -> %.3f', case, index,
             info['P'], info['nb'], nz.min(), nz.max(), info['index_dummies'], info['order_quads_moved'], info['nnz_pad'] // 4, m0, m1)
        assert m1 < m0, (case, m0, m1)
        residues |= set((nz % 64).tolist())
        short += int((nz < 64).sum())
        whole += int((nz > 64).sum())
    if case.startswith('zipf'):
        assert info['P'] == {'zipf-p4': 4, 'zipf-p2': 2, 'zipf-p1': 1}[case], info
        assert info['hot_cols'] > 0, info
    if case == 'short':
        lens = np.diff(raw.indptr)
        assert info['P'] >= 3 and int(((lens > 1) & (lens < info['P'])).sum()) > 1000, 'rows of one and two entries per part, empty cells'
        if index == 2:
            assert info['index_dummies'] > 0.03 * info['nnz_amb'], info
    if case == 'residues':
        assert residues == {0, 16, 32, 48} and short > 0 and whole > 0, (residues, short, whole)


PASS_CASES = [('row_shape_p1', 1, 1, 0), ('row_shape', 2, 1, 0), ('row_shape', 4, 1, 0), ('row_shape_p1', 1, 2, 0), ('row_shape', 2, 2, 0),
              ('row_shape', 4, 2, 0), ('row_shape', 4, 1, 2)]


@pytest.mark.parametrize('mkey,parts,index,geo', PASS_CASES)
def test_passes_against_the_exact_reference(gpu_device, mkey, parts, index, geo):
    raw = E.matrix(mkey, E.REDUCED.get(mkey))
    m = Model(gpu_device, raw, IDX[index] + ON + (('parts', parts), ('geometry', geo)))
    info = _ext(m.eng)
    assert info['P'] == parts and info['geometry'] == geo and info['fused'] == 1 and info['split'] == 0, info
    assert info['index_format'] == index and info['order_kind'] == 2 and info['order_quads_moved'] > 0, info
    top = _leg(m, mkey, ('decades', 'dying'), 'order-%s-P%d-index%d-geo%d' % (mkey, parts, index, geo), forms=False)
    after = _ext(m.eng)
    _say('%s P %d index %d geometry %d: nb %d, %d quads moved | largest: column sums %.3f lnl %.3g diff %.3f', mkey, parts, index, geo, info['nb'],
         info['order_quads_moved'], *top)
    assert after['fallbacks'] == 0 and after['order_kind'] == 2, after


def _four_iterations(raw, options):
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    eng = _lib.Engine(0)
    for k, v in options:
        eng.set_option(k, v)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=4, em_epsilon=0.0))
    tl.em()
    info = _ext(eng)
    mult = []
    for blk in range(2, min(12, info['nb'])):
        for part in range(info['P']):
            mult += _worst(eng.debug_subblock(blk, part, cap=int(info['nnz_pad']) + 64))
    return tl.lnl, tl.pi.copy(), tl.reassign_colsums('exclude'), float(np.mean(mult)), info


@pytest.mark.parametrize('index', [1, 2])
def test_four_iterations_with_the_order_on_and_off(gpu_device, index):
    """the bars of test_conflict_aware_row_order_option: lnl to 1e-12 relative, pi to rtol 1e-11, equal `exclude` counts, and a worst
    multiplicity that falls by more than 0.5"""
    raw = _zipf(30000)
    forced = IDX[index] + (('block_rows', 512), ('geometry', 0))
    off, on = _four_iterations(raw, forced + OFF), _four_iterations(raw, forced + ON)
    assert off[4]['order_kind'] == 0 and on[4]['order_kind'] == 2 and on[4]['index_format'] == index, (off[4], on[4])
    _say('four iterations, index %d: lnl %.15g / %.15g, worst multiplicity %.3f -> %.3f', index, off[0], on[0], off[3], on[3])
    assert abs(off[0] - on[0]) <= 1e-12 * abs(off[0]), (off[0], on[0])
    assert np.allclose(off[1], on[1], rtol=1e-11, atol=0), float(np.max(np.abs(off[1] - on[1]) / np.maximum(off[1], 1e-300)))
    assert np.array_equal(off[2], on[2])
    assert on[3] < off[3] - 0.5, (off[3], on[3])


def _words(eng):
    info = _ext(eng)
    return np.concatenate([w for _, _, w, _, _, _ in _sub_blocks(eng, info)])


def test_the_auto_rule(gpu_device):
    """auto: nothing below 1 GiB of stream (every layout the other test files pin); from `deconflict_min_bytes` on, the quad order"""
    raw = _zipf(30000)
    base = FP64 + (('geometry', 0),)
    _, eng = _load(raw, base)
    info = _ext(eng)
    assert 11 * info['nnz_amb'] < 1 << 30 and info['index_format'] == 1
    assert info['order_kind'] == 0 and info['order_quads_moved'] == 0, info
    _, plain = _load(raw, base + OFF)
    assert np.array_equal(_words(eng), _words(plain)), 'auto below the threshold: the layout words of `deconflict` = 0'
    _, eng = _load(raw, base + (('deconflict_min_bytes', 11 * info['nnz_amb']),))
    low = _ext(eng)
    assert low['order_kind'] == 2 and low['order_quads_moved'] > 0 and low['index_format'] == 1, low
    _, eng = _load(raw, base + (('deconflict_min_bytes', 11 * info['nnz_amb'] + 1),))
    assert _ext(eng)['order_kind'] == 0
    # score codes: the option means what it meant
    _, eng = _load(raw, (('value_format', 2), ('geometry', 0)))
    assert _ext(eng)['order_kind'] == 1 and _ext(eng)['order_quads_moved'] == 0
    _, eng = _load(raw, (('value_format', 2), ('geometry', 0)) + OFF)
    assert _ext(eng)['order_kind'] == 0


KEEP = [FP64 + (('geometry', 0), ('reproducible', 1)), FP64 + (('split', 1), ('parts', 5), ('geometry', 1)), FP64 + (('geometry', 0), ('sorted_fill', 0))]


@pytest.mark.parametrize('options', KEEP, ids=lambda v: '-'.join('%s%d' % kv for kv in v))
def test_what_keeps_its_order(gpu_device, options):
    """`reproducible`, the split layout, the strand-transposed fill: asked for or not, no quad order — and the oracle's results"""
    raw = _zipf(30000)
    for extra in (ON, (('deconflict_min_bytes', 0),)):
        _, eng = _load(raw, options + extra)
        info = _ext(eng)
        assert info['order_kind'] == 0 and info['order_quads_moved'] == 0 and info['fused'] == 1, info
    got = _oracle_vs_gpu(raw, iters=4, options=options + ON)
    assert got['fused'] == 1 and got['fallbacks'] == 0, got


def test_the_two_pass_fall_back_starts_from_the_csr(gpu_device):
    raw = _zipf(30000)
    _, eng = _load(raw, IDX[2] + ON + (('geometry', 0),))
    assert _ext(eng)['order_kind'] == 2
    eng.fallback_twopass()
    info = _ext(eng)
    assert info['fused'] == 0 and info['index_bytes'] == 4 and info['order_kind'] == 0 and info['order_quads_moved'] == 0, info
    got = _oracle_vs_gpu(raw, iters=4, options=IDX[2] + ON + (('geometry', 0), ('fused_dbg', 32)))
    assert got['fused'] == 0 and got['index_bytes'] == 4 and got['fallbacks'] == 1, got
