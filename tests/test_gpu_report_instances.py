"""`-m gpu`: every instance of the streaming report kernels (telescope_amd/csrc/tsem_report.hip, tsem_report_pack.h) against the
exact reference of tests/_report_reference.py, which tests/test_report_reference.py ties down without a GPU.

One matrix per capacity class (8 .. 256 entries per row: `k_report_rows<G, E, INIT, GM>` and `k_report_init_codes<G, E>` at
G x E = 1x8, 1x16, 2x16, 4x16, 8x16, 16x16) and score table (largest score 5 and 400), rows on both sides of every class boundary,
a few rows beyond it (left to k_report_slow) and a last row whose lanes read into the arrays' padding; one matrix with more ids than
k_report_pack32's LDS table holds (`COLD`) and every row length at the steps of its segmented scan.  The engine is set up as `_model`
of tests/test_gpu_rowpass_entries.py does and holds the reference's parameters (eng.set_params).

On every leg:
 1. the launch record (`eng.report_info()`, tsem_report_info_n) names the expected kernel family, lanes per row and entries per lane,
    source of z, group mode and COLD, and its count of rows deferred as too long equals the number of rows longer than G x E
    entries (k_report_pack32: 64 E) — the kernels hand such rows to k_report_slow, so a wrong class or a `>=` for a `>` in the
    deferral shows nowhere else.  (k_report_rows and k_report_init_codes mark the rows they defer as too long, so their count is the
    kernel's own word.  k_report_pack32 stores every deferred row alike and the query tells the long ones by the same 64 E: there
    the count shows that every long row is on the list, not at which length the kernel defers.)  Where k_report_rows keeps only
    part of the popularity ids in LDS (`Hs` accumulator slots, pi*theta of `HC` ids), the matrix has at least 200 columns and 200
    stored entries on either side of each budget, counted from the matrix (_report_reference.ids_beside);
 2. every integer output is bit-equal to the expected one: `exclude`, the tied rows and their counts, the `exclude` / `choose` /
    `unique` / `all` group sums;
 3. every float column (`conf`, `average`) is within its limit (_report_reference: derived from the code, not from any output).

Every leg prints a `REPORT ...` line with the figures it asserts on (`pytest -s`); profiles/r23_report_instances.txt keeps a run and
the legs that caught each of four planted mutations."""
import time

import numpy as np
import pytest

import _report_reference as P
import _rowpass_reference as R
import test_gpu_rowpass_entries as E

pytestmark = pytest.mark.gpu
INSTANCE = {8: (1, 8), 16: (1, 16), 32: (2, 16), 64: (4, 16), 128: (8, 16), 256: (16, 16)}      # class -> lanes per row, entries per lane
GROUP_MODE = {'exclude': 1, 'average': 2, 'conf': 3, 'all': 4}
INTEGER_METHODS = ('exclude', 'choose', 'unique', 'all')
CASES = [(c, s) for c in P.CLASSES for s in P.SCORES]


def _say(fmt, *a):
    print('REPORT ' + fmt % a, flush=True)


def _dev(which):
    from telescope_amd import _lib
    return _lib.Z_INITIAL if which == R.INITIAL else _lib.Z_CUR


def _engine(gpu_device, case):
    raw, lut, pi, theta = case
    eng, _ = E._model(gpu_device, raw, lut)
    eng.set_params(pi, theta)
    return eng


def _check_sums(got, ref, method, thresh, label, keep=None):
    """check 2 or 3 on one vector of column sums; returns the fraction of the limit"""
    want, lim = ref.sums(method, thresh, keep)
    if method in INTEGER_METHODS:
        bad = np.flatnonzero(got != want.astype(np.float64))
        assert len(bad) == 0, (label, method, 'columns', bad[:5], got[bad[:5]], want[bad[:5]].astype(np.float64))
        return 0.0
    frac = P.fraction(got, want, lim)
    assert frac <= 1.0, (label, method, 'fraction of the limit', frac, int(np.argmax(np.abs(got - want.astype(np.float64)))))
    return frac


def _check_record(info, label, kernel, g, e, initial, group_mode=0, cold=None, too_long=None):
    """check 1"""
    got = (info['kernel'], info['G'], info['E'], info['initial'], info['group_mode'])
    assert got == (kernel, g, e, int(initial), group_mode), (label, got, (kernel, g, e, int(initial), group_mode))
    assert info['grid'] > 0 and info['block'] in (256, 512, 1024), (label, info)
    if cold is not None:
        assert info['cold'] == cold, (label, info)
    if too_long is not None:
        assert info['deferred_long'] == too_long, (label, 'rows deferred as too long', info['deferred_long'], 'rows beyond G x E', too_long)
        assert info['deferred_near'] >= 0, (label, info)


def _check_ids(info, raw, lay, label, cap, least=200):
    """k_report_rows: the LDS paths (id < Hs, id < HC) and the global ones (the rest) both meet stored entries of this matrix"""
    out = []
    for name in ('Hs',) if info['initial'] else ('Hs', 'HC'):
        inside, outside = P.ids_beside(raw, info[name], lay['P'], lay['hot_cols'], cap)
        assert min(inside) >= least and min(outside) >= least, (label, name, info[name], 'inside', inside, 'outside', outside)
        out.append('%s %d: %d entries on %d columns inside, %d on %d outside' % (name, info[name], inside[1], inside[0], outside[1], outside[0]))
    _say('%s: ids beside the LDS budgets, at least: %s', label, '; '.join(out))


def _colsums_leg(eng, ref, thresh, label, kernel, g, e, cold=None):
    """one tsem_report_colsums (thresh < 0: no `conf` column, the others as at 0.9) against the reference"""
    t0 = time.time()
    sums, rows, counts = eng.report_colsums(_dev(ref.which), thresh)
    dt = time.time() - t0
    info = eng.report_info()['colsums']
    cap = (64 if kernel == 'k_report_pack32' else g) * e
    _check_record(info, label, kernel, 64 if kernel == 'k_report_pack32' else g, e, ref.which == R.INITIAL, 0, cold,
                  int(np.count_nonzero(ref.lens > cap)))
    assert eng.report_stats()['kernel'] == kernel, (label, eng.report_stats())
    if kernel == 'k_report_rows':
        _check_ids(info, ref.raw, eng.layout_info(), label, cap)
    t = 0.9 if thresh < 0 else thresh
    want_rows, want_counts = ref.ties(t)
    assert np.array_equal(rows, want_rows) and np.array_equal(counts, want_counts), (label, 'tied rows')
    _check_sums(sums['exclude'], ref, 'exclude', t, label)
    fa = _check_sums(sums['average'], ref, 'average', t, label)
    # (thresh < 0: that third is "not meaningful" by telescope_em.h — k_report_slow adds the deferred rows' conf at 0.9 to it, the
    # kernels other than k_report_init_codes all of it — so nothing is asserted on it)
    fc = 0.0 if thresh < 0 else _check_sums(sums['conf'], ref, 'conf', t, label)
    _say('%s: %s<%d, %d> Hs %d HC %d lut_rep %d grid %d x %d, %d rows too long, %d near-ties, %d tied rows; conf %.3f average %.3f of the limit; %.1f ms',
         label, kernel, info['G'], info['E'], info['Hs'], info['HC'], info['lut_rep'], info['grid'], info['block'], info['deferred_long'],
         info['deferred_near'], len(rows), fc, fa, 1e3 * dt)
    return sums, rows, counts, info


@pytest.mark.parametrize('c,max_score', CASES)
def test_column_sums_of_every_instance(gpu_device, c, max_score):
    g, e = INSTANCE[c]
    eng = _engine(gpu_device, P.class_case(c, max_score))
    ini, cur = P.reference(c, max_score, R.INITIAL), P.reference(c, max_score, R.CUR)
    tag = 'class %d, scores to %d' % (c, max_score)
    e_pack = 16 if ini.raw.nnz >= 24 * ini.raw.shape[0] else 8
    _colsums_leg(eng, ini, 0.9, tag + ', initial z with conf', 'k_report_rows', g, e)
    _colsums_leg(eng, ini, -1.0, tag + ', initial z without conf', 'k_report_init_codes', g, e)
    info = _colsums_leg(eng, cur, 0.9, tag + ', final z at 0.9', 'k_report_pack32', 64, e_pack, cold=0)[3]
    assert info['HC'] >= P.K and info['Hs'] == 0, (tag, info)            # every id's pi*theta in LDS
    for dbg, ee in ((128, 8), (256, 16)):
        eng.set_option('report_dbg', dbg)
        _colsums_leg(eng, cur, 0.9, tag + ', final z at 0.9, report_dbg %d' % dbg, 'k_report_pack32', 64, ee, cold=0)
    eng.set_option('report_dbg', 8)
    info = _colsums_leg(eng, cur, 0.9, tag + ', final z at 0.9, report_dbg 8', 'k_report_rows', g, e)[3]
    assert 0 < info['Hs'] <= 3072 < info['HC'] < P.K, (tag, info)                     # (the ids beside them: _check_ids, every leg)
    eng.set_option('report_dbg', 0)
    for thresh in (0.45, 0.5, 1.0):
        _colsums_leg(eng, cur, thresh, tag + ', final z at %.2f' % thresh, 'k_report_rows', g, e)
    if c in (16, 128):                                                                # option `reproducible`: exact split sums
        eng.set_option('reproducible', 1)
        for ref, thresh, what in ((cur, 0.9, 'final z at 0.9'), (ini, 0.9, 'initial z with conf'), (ini, -1.0, 'initial z without conf')):
            a = _colsums_leg(eng, ref, thresh, tag + ', reproducible, ' + what, 'k_report_rows', g, e)
            b = eng.report_colsums(_dev(ref.which), thresh)
            for m in P.REPORT_METHODS:
                assert np.array_equal(a[0][m], b[0][m]), (tag, what, m, 'two reproducible calls differ')
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (tag, what)
        eng.set_option('reproducible', 0)
    eng.close()


@pytest.mark.parametrize('c,max_score', CASES)
def test_group_sums_of_every_instance(gpu_device, c, max_score):
    g, e = INSTANCE[c]
    eng = _engine(gpu_device, P.class_case(c, max_score))
    n, k = P.N_ROWS, P.K
    lay = eng.layout_info()
    idn = lay['P'] * lay['Kp']
    group = P.group_map(n)
    tag = 'class %d, scores to %d' % (c, max_score)
    # the two calls share the deferred list: k_group_unique leaves it alone, a streaming group pass takes it over
    eng.report_colsums(_dev(R.INITIAL), -1.0)
    first = eng.report_info()['colsums']
    assert first['deferred_long'] == np.count_nonzero(P.reference(c, max_score, R.INITIAL).lens > g * e), (tag, first)
    eng.reassign_groups('unique', 0.9, _dev(R.INITIAL), group, P.GROUPS)
    assert eng.report_info()['colsums'] == first, (tag, eng.report_info())
    eng.reassign_groups('exclude', 0.9, _dev(R.INITIAL), group, P.GROUPS)
    both = eng.report_info()
    assert both['colsums']['deferred_long'] == -1 and both['groups']['deferred_long'] >= 0, (tag, both)
    seen = set()
    for which in (R.INITIAL, R.CUR):
        ref = P.reference(c, max_score, which)
        per_tile = 1 if (which == R.INITIAL) == (max_score == 5) else 2              # streamed groups per tile: both occur per class and z
        budget = per_tile * (k + idn) * 8 + 8
        eng.set_option('group_tile_bytes', budget)
        for m in R.METHODS:
            label = '%s, %s z, groups, %s' % (tag, which, m)
            stream = m in GROUP_MODE
            tile = max(1, min(P.GROUPS, budget // ((k + (idn if stream else 0)) * 8)))
            t0 = time.time()
            got = eng.reassign_groups(m, 0.9, _dev(which), group, P.GROUPS, ref.picks if m == 'choose' else None)
            dt = time.time() - t0
            info = eng.report_info()['groups']
            last = np.arange(n)[(group >= (P.GROUPS - 1) // tile * tile)]            # rows of the last tile's groups
            if stream:
                _check_record(info, label, 'k_report_rows', g, e, which == R.INITIAL, GROUP_MODE[m],
                              too_long=int(np.count_nonzero(ref.lens[last] > g * e)))
                seen.add(info['tile_groups'])
            else:
                assert info['kernel'] == ('k_group_unique' if m == 'unique' else 'k_rowpass') and info['deferred_long'] == -1, (label, info)
            assert (info['tiles'], info['tile_groups']) == (-(-P.GROUPS // tile), P.GROUPS - (P.GROUPS - 1) // tile * tile), (label, info, tile)
            frac = max(_check_sums(got[q], ref, m, 0.9, label + ', group %d' % q, group == q) for q in range(P.GROUPS))
            _say('%s: %s gm %d, %d tiles, %d rows of the last tile too long; %.3f of the limit; %.1f ms', label, info['kernel'],
                 info['group_mode'], info['tiles'], info['deferred_long'], frac, 1e3 * dt)
    assert seen == {1, 2}, (tag, 'streamed groups in the last tile', seen)
    eng.close()


def test_packed_kernel_with_cold_ids(gpu_device):
    """48 000 columns: the table of the ids does not fit k_report_pack32's LDS (`COLD`: the tail is gathered from L2), and every row
    length at which its segmented scan takes another step, for 8 and for 16 entries per lane.  k_report_rows<16, 16> then serves
    the same matrix (report_dbg 8), and its group instances do (tsem_reassign_groups, the four streamed methods): two thirds of the
    ids lie outside their tables of pi*theta."""
    raw = P.cold_case()[0]
    eng = _engine(gpu_device, P.cold_case())
    cur = P.reference('cold', 400, R.CUR)
    lay = eng.layout_info()
    idn = lay['P'] * lay['Kp']
    e_pack = 16 if raw.nnz >= 24 * raw.shape[0] else 8
    for dbg, ee in ((0, e_pack), (128, 8), (256, 16)):
        eng.set_option('report_dbg', dbg)
        info = _colsums_leg(eng, cur, 0.9, 'COLD matrix, final z at 0.9, report_dbg %d' % dbg, 'k_report_pack32', 64, ee, cold=1)[3]
        assert 0 < info['HC'] < idn <= 65536, (info, idn)
        assert len(np.unique(raw.indices)) > info['HC'], (info, 'no id outside the LDS table is in use')
    eng.set_option('report_dbg', 8)
    info = _colsums_leg(eng, cur, 0.9, 'COLD matrix, final z at 0.9, report_dbg 8', 'k_report_rows', 16, 16)[3]
    assert 0 < info['Hs'] <= 3072 < info['HC'] < idn // 2, (info, idn)
    eng.set_option('report_dbg', 0)
    # the group instances k_report_rows<16, 16, false, 1 .. 4>: with the class matrices pi*theta of every id in use fits their LDS
    # (HC about 20 000 there); here two thirds of the ids lie outside, so their global gather runs too.  Two groups per tile.
    n = raw.shape[0]
    group = P.group_map(n)
    eng.set_option('group_tile_bytes', 2 * (P.K_COLD + idn) * 8 + 8)
    last = group >= P.GROUPS - 2
    for m in sorted(GROUP_MODE, key=GROUP_MODE.get):
        label = 'COLD matrix, final z, groups, %s' % m
        t0 = time.time()
        got = eng.reassign_groups(m, 0.9, _dev(R.CUR), group, P.GROUPS)
        dt = time.time() - t0
        info = eng.report_info()['groups']
        _check_record(info, label, 'k_report_rows', 16, 16, False, GROUP_MODE[m], too_long=int(np.count_nonzero(cur.lens[last] > 256)))
        assert (info['tiles'], info['tile_groups']) == (2, 2) and 0 < info['HC'] < idn // 2, (label, info)
        inside, outside = P.ids_beside(raw, info['HC'], lay['P'], lay['hot_cols'], 256)
        assert min(inside) >= 200 and min(outside) >= 200, (label, info['HC'], inside, outside)
        frac = max(_check_sums(got[q], cur, m, 0.9, label + ', group %d' % q, group == q) for q in range(P.GROUPS))
        _say('%s: %s gm %d HC %d (at least %d entries on %d columns outside), %d tiles, %d rows of the last tile too long; %.3f of the limit; %.1f ms',
             label, info['kernel'], info['group_mode'], info['HC'], outside[1], outside[0], info['tiles'], info['deferred_long'], frac, 1e3 * dt)
    eng.close()
