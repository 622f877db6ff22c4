"""`-m gpu`: the 8-byte quad index of the fused layouts with fp64 entries (telescope_amd/csrc/tsem_quad64.h; option `index_format` = 2):
2 B of index per entry, 10 B per entry in the stream of the fused EM / lnl passes.

  layout      against the 3-byte layout of the same matrix: the same stored entries, the same (row slot, column slot) pairs per sub-block
              once the dummies are set aside, rows ascending by steps of 0 or 1, every row of a block present in every part, the
              accounting identities, column bit 12 and row bit 8 in use; a matrix with many empty (row, part) cells;
  passes      one EM pass, one lnl pass in every form, the update and the passes after it against the long-double reference of
              tests/_em_pass_reference.py with its own bounds (the legs of tests/test_gpu_em_pass_exact.py): teams of 1, 4 and 8, fp64
              row weights and row weight codes (FMT 0 / 2), hot columns on and off, sub-blocks of every quad count modulo 64, rings
              that wrap twice;
  the loop    four iterations against the oracle, with `use_likelihood`, and through an injected hand-off time-out;
  the choice  what keeps its index, and the auto rule with its size threshold lowered.

Planted mutations (each planted once, one line, and seen to fail the legs named; profiles/r28_quad_index.txt section 9):
  a step bit ignored in the decode (ts_quad64_row without d2) — every leg of test_passes_against_the_exact_reference,
      test_four_iterations_against_the_oracle, test_layout_against_the_three_byte_layout; the host decoder shares the function, so
      tests/test_quad64_host.py fails too (test_word_against_the_model, test_every_column_bit_and_every_row_bit);
  the dummy written to column 0 of the WRONG row (row slot lr + 1) — test_many_empty_cells, test_layout_against_the_three_byte_layout
      and test_the_auto_rule: the pack kernel counts quads it cannot represent, the layout keeps 3 bytes, `_assert_quad` fails;
  the pack kernel reading quad t + 1 — test_layout_against_the_three_byte_layout and test_many_empty_cells (rows no longer ascend
      across quads, values no longer belong to the cells the index names), every leg of test_passes_against_the_exact_reference
      and test_four_iterations_against_the_oracle."""
import numpy as np
import pytest

import _em_pass_reference as E
from test_gpu_em_pass_exact import Model, _leg, _ring_rows, cu_count  # noqa: F401  (cu_count: a fixture)
from test_gpu_idx24 import _load, _short_rows, _zipf
from test_gpu_parity import RTOL, _oracle_vs_gpu

pytestmark = pytest.mark.gpu
QUAD = (('value_format', 1), ('index_format', 2))


def _say(fmt, *a):
    print('QUAD64 ' + fmt % a, flush=True)


def _ext(eng):
    return eng.layout_info(extended=True)


def _assert_quad(info, label=''):
    assert info['fused'] == 1 and info['split'] == 0 and info['row_order'] == 1 and info['value_bytes'] == 8, (label, info)
    assert info['index_unrepresentable'] == 0, (label, 'the pack kernel met quads it cannot represent', info)
    assert info['index_bytes'] == 2 and info['index_format'] == 2, (label, info)


def _sub_blocks(eng, info, K):
    """every sub-block of a layout with fp64 entries: (block, part, words, values, CSR rows, CSR columns)"""
    cap = int(info['nnz_pad']) + 64
    for blk in range(info['nb']):
        for part in range(info['P']):
            w = eng.debug_subblock(blk, part, cap=cap)
            v, rows, cols = eng.debug_subblock_values(blk, part, cap=cap)
            assert len(v) == len(w) and len(w) % 64 == 0 and len(w) < cap
            yield blk, part, w, v, rows, cols


def _check_quad_layout(eng, raw, lut, label):
    """What the format promises of a layout, from the decoders alone.  Returns (step patterns seen, column bit 12 seen, row bit 8 seen,
    dummies found, quad counts)."""
    info = _ext(eng)
    _assert_quad(info, label)
    K = raw.shape[1]
    key_all = raw.indices.astype(np.int64) + np.repeat(np.arange(raw.shape[0], dtype=np.int64), np.diff(raw.indptr)) * K
    want_all = lut[raw.data]
    patterns, hi_col, hi_row, nonreal, seen, nqs = set(), False, False, 0, [], []
    parts_of_row = np.zeros(raw.shape[0], np.int64)                  # bit q: the row has a real entry in part q
    rows_in_block = {}
    for blk, part, w, v, rows, cols in _sub_blocks(eng, info, K):
        nqs.append(len(w) // 4)
        if len(w) == 0:
            continue
        lr, lc = (w >> 16).astype(np.int64), (w & 0xFFFF).astype(np.int64)
        assert lr.max() < info['R'] and lc.max() < info['Kp'], (label, blk, part)
        d = np.diff(lr)
        assert np.all((d == 0) | (d == 1)), (label, blk, part, 'rows ascend by steps of 0 or 1')
        assert lr[0] == 0, (label, blk, part, 'a sub-block starts with row slot 0')
        rows_in_block.setdefault(blk, set()).add(int(lr.max()))
        q = lr.reshape(-1, 4)
        patterns |= set(map(tuple, np.diff(q, axis=1).tolist()))
        hi_col |= bool((lc >= 4096).any())
        hi_row |= bool((lr >= 256).any())
        real = v != 0.0
        assert np.all(lc[~real] == 0), (label, blk, part, 'dummies and padding sit in column slot 0')
        nonreal += int((~real).sum())
        key = rows[real].astype(np.int64) * K + cols[real]
        at = np.searchsorted(key_all, key)
        assert np.all(at < len(key_all)) and np.array_equal(key_all[np.minimum(at, len(key_all) - 1)], key), \
            (label, blk, part, 'an index word names a cell the matrix does not store')
        assert np.array_equal(v[real].view(np.uint64), want_all[at].view(np.uint64)), (label, blk, part, 'values out of place')
        np.bitwise_or.at(parts_of_row, rows[real], 1 << part)
        seen.append(key)
    for blk, tops in rows_in_block.items():
        assert len(tops) == 1, (label, blk, 'every row of the block in every part: the parts end on different rows', tops)
    seen = np.concatenate(seen)
    assert len(seen) == info['nnz_amb'] and len(np.unique(seen)) == len(seen), (label, 'every stored entry once', len(seen), info['nnz_amb'])
    amb = np.diff(raw.indptr) > 1
    empty_cells = int(sum(int(((parts_of_row[amb] >> q) & 1 == 0).sum()) for q in range(info['P'])))
    assert info['index_dummies'] == empty_cells, (label, 'dummies', info['index_dummies'], empty_cells)
    assert nonreal == info['nnz_pad'] - info['nnz_amb'] and nonreal >= empty_cells, (label, nonreal, info['nnz_pad'], info['nnz_amb'], empty_cells)
    # the accounting: 10 B per entry in the stream, (2 + 8) B per padded entry resident
    assert eng.kernel_stats()['algo_bytes_per_pass'] == 10 * info['nnz_amb'] + 2 * info['N_amb'], label
    assert eng.device_memory()['resident']['layout'] == (2 + 8) * info['nnz_pad'] + 12 * (info['nb'] * info['P'] + 2), label
    return patterns, hi_col, hi_row, empty_cells, np.array(nqs)


ALL_PATTERNS = {(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)}


def test_layout_against_the_three_byte_layout(gpu_device):
    """60 000 x 30 000 x ~24, teams of 4, Kp ~ 7500 (column bit 12), 512 row slots with more than 256 rows in a block (row bit 8)"""
    raw = _zipf(30000)
    from telescope_amd.likelihood import score_lut
    lut = score_lut(int(raw.data.max()))
    forced = (('block_rows', 512), ('geometry', 0))
    _, a = _load(raw, QUAD + forced)
    _, b = _load(raw, (('value_format', 1), ('index_format', 1)) + forced)
    ia, ib = _ext(a), _ext(b)
    assert ib['index_bytes'] == 3 and ib['index_format'] == 1 and ib['index_dummies'] == 0
    assert [ia[k] for k in ('P', 'Kp', 'R', 'N_amb', 'nnz_amb')] == [ib[k] for k in ('P', 'Kp', 'R', 'N_amb', 'nnz_amb')]
    assert ia['P'] == 4 and ia['Kp'] > 4096 and ia['R'] == 512
    patterns, hi_col, hi_row, dummies, nqs = _check_quad_layout(a, raw, lut, 'zipf')
    assert hi_col and hi_row and patterns == ALL_PATTERNS, (hi_col, hi_row, patterns)
    assert 0 < dummies <= 0.005 * ia['nnz_amb'], (dummies, ia['nnz_amb'])
    # sub-block by sub-block wherever the two layouts cut the same blocks (the dummies count towards a block's capacity, so a
    # boundary may move): the same (row slot, column slot) pairs once the dummies and the padding (value 0) are set aside
    K, same = raw.shape[1], 0
    hot = 0
    for (blk, part, wa, va, ra, ca), (_, _, wb, vb, rb, cb) in zip(_sub_blocks(a, ia, K), _sub_blocks(b, ib, K)):
        fa, fb = va != 0.0, vb != 0.0
        if int(fa.sum()) != int(fb.sum()) or not np.array_equal(np.unique(ra[fa]), np.unique(rb[fb])):
            continue
        # the same rows: the same cells of the matrix, in the same order (a row's entries keep their CSR order inside a part)
        assert np.array_equal(ra[fa], rb[fb]) and np.array_equal(ca[fa], cb[fb]), (blk, part)
        if ra[0] == rb[0]:
            # ... and the same first row: the same row slots.  The column slots agree but for the hot columns, whose entries are dealt
            # over their slots by position in the sub-block — and a dummy in front moves the position
            assert np.array_equal(wa[fa] >> 16, wb[fb] >> 16), (blk, part)
            differ = (wa[fa] & 0xFFFF) != (wb[fb] & 0xFFFF)
            hot += int(differ.sum())
            for col in np.unique(ca[fa][differ]):
                slots = np.unique(np.concatenate([(wa[fa] & 0xFFFF)[ca[fa] == col], (wb[fb] & 0xFFFF)[cb[fb] == col]]))
                assert len(slots) > 1 and slots.max() - slots.min() < 16, (blk, part, col, slots)
        same += 1
        if blk >= 20:
            break
    assert same >= ia['P'], ('no block of the two layouts holds the same rows', same)
    _say('zipf 60k x 30k: nb %d / %d, %d dummies of %d entries, %d sub-blocks compared pair by pair, quads %d .. %d', ia['nb'], ib['nb'], dummies,
         ia['nnz_amb'], same, nqs.min(), nqs.max())
    assert ia['hot_cols'] > 0
    assert b.device_memory()['resident']['layout'] - (3 + 8) * ib['nnz_pad'] == 12 * (ib['nb'] * ib['P'] + 2)


def test_many_empty_cells(gpu_device):
    """rows of 2 - 6 entries over 16 000 columns: most rows miss a part.  Every in-quad step pattern occurs, the dummies are counted,
    nothing is unrepresentable."""
    raw = _short_rows()
    from telescope_amd.likelihood import score_lut
    _, eng = _load(raw, QUAD + (('geometry', 0), ('block_rows', 512)))
    info = _ext(eng)
    P = info['P']
    lens = np.diff(raw.indptr)
    assert P >= 3 and int(((lens > 1) & (lens < P)).sum()) > 1000, 'rows with fewer entries than parts: each has an empty part'
    assert info['geometry'] == 0 and info['R'] == 512
    patterns, _, hi_row, dummies, nqs = _check_quad_layout(eng, raw, score_lut(int(raw.data.max())), 'short')
    assert patterns == ALL_PATTERNS and hi_row, patterns
    assert dummies > 0.03 * info['nnz_amb'], (dummies, info['nnz_amb'])
    _say('short rows: P %d nb %d, %d dummies beside %d entries (%.1f %%), quads %d .. %d', P, info['nb'], dummies, info['nnz_amb'],
         100.0 * dummies / info['nnz_amb'], nqs.min(), nqs.max())


# ---- one EM pass, one lnl pass in every form, the update, the passes after it ---------------------------------------------------------
def _big_lut(raw):
    """the model's table behind 3000 entries: too long for LDS, so the fused kernel reads fp64 row weights (FMT 0)"""
    t = E.lut(raw)
    return np.concatenate([t, np.repeat(t[-1], 3000 - len(t))])


PASS_CASES = [('row_shape_p1', 1, 2, ()), ('row_shape', 4, 2, ()), ('row_shape', 8, 2, ()),
              ('row_shape_p1', 1, 0, ()), ('row_shape', 4, 0, ()), ('row_shape', 8, 0, ()),
              ('zipf', 4, 2, (('hot_split', 1),)), ('zipf', 4, 2, (('hot_split', 0),)),
              ('row_shape', 4, 2, (('block_rows', 64),)), ('short', 3, 2, (('geometry', 0), ('block_rows', 512)))]


@pytest.mark.parametrize('mkey,parts,fmt,extra', PASS_CASES, ids=lambda v: '-'.join('%s%d' % kv for kv in v) if isinstance(v, tuple) else str(v))
def test_passes_against_the_exact_reference(gpu_device, mkey, parts, fmt, extra):
    raw = E.matrix(mkey, E.REDUCED.get(mkey))
    # (the geometry is forced: left alone, rows this short take the geometries of 768 row slots, which keep the 3-byte index)
    geo = () if 'geometry' in dict(extra) else (('geometry', 1 if parts > 4 else 0),)
    m = Model(gpu_device, raw, QUAD + (('parts', parts),) + geo + extra, lut=_big_lut(raw) if fmt == 0 else None)
    info = _ext(m.eng)
    _assert_quad(info, (mkey, parts, fmt, extra))
    assert info['P'] == parts and info['geometry'] == (1 if parts > 4 else 0), info
    assert info['lds_bytes'] > 0
    if 'hot_split' in dict(extra):
        assert (info['hot_cols'] > 0) == (dict(extra)['hot_split'] == 1), info
    top = _leg(m, (mkey, E.REDUCED.get(mkey)) if mkey in E.REDUCED else mkey, ('decades', 'dying'), 'quad-%s-P%d-fmt%d' % (mkey, parts, fmt), forms=fmt != 0)
    after = _ext(m.eng)
    _say('%s P %d FMT %d %s: nb %d R %d dummies %d | largest: column sums %.3f lnl %.3g diff %.3f', mkey, parts, fmt, dict(extra), info['nb'], info['R'],
         info['index_dummies'], *top)
    assert after['fallbacks'] == 0 and after['index_bytes'] == 2, after


def test_sub_blocks_of_every_quad_count_modulo_64(gpu_device):
    """block_rows = 64: the sub-blocks have 16, 32, 48 and 0 quads modulo the value map's group of 64, and some are shorter than a group"""
    residues, short, whole = set(), 0, 0
    for mkey, parts in (('ring', 1), ('row_shape', 4)):
        raw = E.matrix(mkey, E.REDUCED.get(mkey))
        m = Model(gpu_device, raw, QUAD + (('parts', parts), ('geometry', 0), ('block_rows', 64)))
        nqs = _check_quad_layout(m.eng, raw, m.lut, mkey)[4]
        nz = nqs[nqs > 0]
        residues |= set((nz % 64).tolist())
        short += int((nz < 64).sum())
        whole += int((nz > 64).sum())
        _leg(m, (mkey, E.REDUCED.get(mkey)) if mkey in E.REDUCED else mkey, ('decades',), 'quad-r64-%s' % mkey, forms=False)
    assert residues == {0, 16, 32, 48}, residues
    assert short > 0 and whole > 0, (short, whole)


@pytest.mark.parametrize('parts', [4, 8])
def test_rings_wrap_twice(gpu_device, cu_count, parts):  # noqa: F811
    """every team walks at least 17 blocks: the six register sets and the eight exchange slots wrap twice"""
    need, teams, rows = _ring_rows(cu_count, parts)
    raw = E.matrix('ring', rows)
    m = Model(gpu_device, raw, QUAD + (('parts', parts), ('geometry', 1 if parts > 4 else 0), ('block_rows', 64)))
    info = _ext(m.eng)
    _assert_quad(info, parts)
    assert need >= 17 and info['nb'] // teams >= need, (info, teams)
    top = _leg(m, ('ring', rows), ('decades',), 'quad-ring-P%d' % parts, forms=False)
    _say('ring P %d: %d rows, %d blocks over %d teams, dummies %d | largest: column sums %.3f lnl %.3g diff %.3f', parts, rows, info['nb'], teams,
         info['index_dummies'], *top)
    assert _ext(m.eng)['fallbacks'] == 0


# ---- the loop -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cols,parts', [(5000, 1), (30000, 4), (60000, 8)])
def test_four_iterations_against_the_oracle(gpu_device, cols, parts):
    info = _oracle_vs_gpu(_zipf(cols), iters=4, options=QUAD + (('geometry', 1 if parts > 4 else 0),))
    assert info['P'] == parts and info['fused'] == 1 and info['split'] == 0 and info['index_bytes'] == 2 and info['fallbacks'] == 0, info


def test_use_likelihood_loop(gpu_device):
    """`--use_likelihood`: the stopping rule reads the log-likelihood of every iteration (fp64 entries: the dedicated lnl pass)"""
    from oracle.telescope_oracle import OracleModel
    raw = _zipf(30000)
    tl, eng = _load(raw, QUAD + (('geometry', 0),))
    tl.max_iter = 4
    tl._raw = raw
    tl.em(use_likelihood=True)
    om = OracleModel(raw)
    om.em(0.0, 4, use_likelihood=True)
    assert _ext(eng)['index_bytes'] == 2
    assert abs(tl.lnl - om.lnl) <= RTOL * abs(om.lnl)
    assert np.allclose(tl.pi, om.pi, rtol=RTOL, atol=0) and np.allclose(tl.theta, om.theta, rtol=RTOL, atol=0)


def test_fall_back_from_a_quad_layout_rebuilds_the_32_bit_index(gpu_device):
    """fused_dbg = 32: the first EM pass reports a hand-off time-out; the rebuild for the two-pass kernels starts from the CSR — no
    dummies, the 32-bit index — and the run ends where the oracle ends"""
    info = _oracle_vs_gpu(_zipf(30000), iters=4, options=QUAD + (('geometry', 0), ('fused_dbg', 32)))
    assert info['fused'] == 0 and info['index_bytes'] == 4 and info['fallbacks'] == 1, info


# ---- the choice -----------------------------------------------------------------------------------------------------------------------
KEEP = [((('value_format', 1), ('geometry', 0), ('reproducible', 1)), 3), ((('value_format', 1), ('geometry', 0), ('sorted_fill', 0)), 3),
        ((('value_format', 2), ('geometry', 0)), 4), ((('value_format', 1), ('split', 1), ('parts', 5), ('geometry', 1)), 4),
        ((('value_format', 1), ('geometry', 2)), 3)]


@pytest.mark.parametrize('options,index_bytes', KEEP, ids=lambda v: '-'.join('%s%d' % kv for kv in v) if isinstance(v, tuple) else str(v))
def test_what_keeps_its_index(gpu_device, options, index_bytes):
    """option `reproducible`, the strand-transposed fill, score codes, the split layout and the geometries of more than 512 row slots:
    auto leaves them alone even with its size rule out of the way, and forcing the quad index fails with a text"""
    from telescope_amd import _lib
    raw = _zipf(30000)
    _, eng = _load(raw, options + (('index_auto_min_bytes', 0),))
    info = _ext(eng)
    assert info['index_bytes'] == index_bytes and info['index_format'] == (1 if index_bytes == 3 else 0) and info['index_dummies'] == 0, info
    with pytest.raises(_lib.EngineError) as ei:
        _load(raw, options + (('index_format', 2),))
    assert 'index_format=2' in str(ei.value), str(ei.value)


def test_the_auto_rule(gpu_device):
    """auto: not on matrices whose stream is below 1 GiB (every layout the other test files pin); with the threshold lowered, where the
    dummies stay within 0.5 % of the entries and not beyond"""
    raw = _zipf(30000)
    base = (('value_format', 1), ('geometry', 0))
    _, eng = _load(raw, base)
    info = _ext(eng)
    assert info['index_auto_min_bytes'] == 1 << 30 and 11 * info['nnz_amb'] < 1 << 30
    assert info['index_bytes'] == 3 and info['index_format'] == 1 and info['index_dummies'] == 0, info
    _, eng = _load(raw, base + (('index_auto_min_bytes', 11 * info['nnz_amb']),))
    low = _ext(eng)
    _assert_quad(low)
    assert 0 < low['index_dummies'] <= 0.005 * low['nnz_amb'], low
    _, eng = _load(raw, base + (('index_auto_min_bytes', 11 * info['nnz_amb'] + 1),))
    assert _ext(eng)['index_bytes'] == 3
    # rows of 2 - 6 entries: far more dummies than 0.5 % — auto declines, whatever the size rule says
    _, eng = _load(_short_rows(), (('value_format', 1), ('geometry', 0), ('block_rows', 512), ('index_auto_min_bytes', 0)))
    short = _ext(eng)
    assert short['index_bytes'] == 3 and short['index_format'] == 1 and short['index_dummies'] == 0 and short['geometry'] == 0, short
    _say('auto: zipf %d dummies of %d entries taken; short rows declined', low['index_dummies'], low['nnz_amb'])
