"""No GPU: the inputs of tests/test_gpu_setup_products.py are fair, and tests/_setup_reference.py is what it says.

 * on every matrix and table the GPU file uses, the emulated level split leaves nothing over and lies within (PIS_LEVELS - 1) 2^-53
   of the exact sum; math.fsum is the exact integer sum, correctly rounded;
 * no two columns that are not twins hold equally many entries and the same modelled 32-bit hash — whole matrices and the shards with
   their row offsets —, so the device's classes must equal the true classes exactly;
 * every matrix lands in the k_rowstats<G> / k_colsig<G> it was built for, holds the lengths and the marked rows it promises;
 * E.twin_representatives on the modelled (count, hash) gives the true classes;
 * the table past the levels' range, once: what the split without a remainder drops, and what the contract allows."""
import math

import numpy as np
import pytest

import _em_pass_reference as E
import _setup_reference as S

NAMES = S.MATRICES


@pytest.mark.parametrize('name', NAMES)
def test_tables_and_level_split_are_fair(name):
    b = S.matrix(name)
    assert S.table_is_fair(b.lut) and b.lut[0] == 0.0 and S.table_span(b.lut) <= S.PIS_EXACT_SPAN
    assert int(b.raw.data.max()) < len(b.lut)
    p = S.Pisum0(b.raw, b.lut)
    assert p.left.max() == 0.0 and not p.remainder_exceeds_q           # nothing is left over
    assert np.array_equal(p.kept(), p.emulated)
    frac, j = p.worst(p.emulated)
    assert frac <= 1.0, (name, j, frac)
    for c in np.flatnonzero(p.n):                                       # fsum = the exact integer sum, correctly rounded
        assert p.exact[c] == p.exact_units[c] / (1 << 1074), (name, c)
    assert np.array_equal(p.emulated == 0, ~p.positive)
    assert p.level_pieces < 1 << S.PIS_W                                # (far from where a level's sum stops being exact)
    print('SETUP-REF %s: emulation %.3f of the bound, %d of %d columns differ from fsum, at most %d pieces in a level'
          % (name, frac, int((p.emulated != p.exact).sum()), int((p.n > 0).sum()), p.level_pieces))


def test_big_column_takes_both_ends_of_the_table():
    b = S.matrix('big_column')
    col, code = S.unique_rows(b.raw)
    mine = code[col == 5]
    assert len(mine) == S.BIG_COLUMN_ROWS and mine.min() < 40 and mine.max() == 65535 and (mine > 65000).sum() > 5000 and (mine < 40).sum() > 5000
    assert set(code[col == 6]) <= {1, 2, 3} and (col == 6).sum() == 300


@pytest.mark.parametrize('name', NAMES)
def test_signatures_tell_all_columns_apart(name):
    b = S.matrix(name)
    assert S.colliding_columns(b.raw) == []
    cnt, h32 = S.signature(b.raw)
    rep, n_twin = S.true_twins(b.raw)
    assert np.array_equal(E.twin_representatives(cnt, h32), rep)
    assert n_twin == int((np.bincount(rep, minlength=len(rep))[rep] > 1).sum())
    for c in b.empty:
        assert cnt[c] == 0 and rep[c] == c


def test_hash_model_scalar_and_vector_agree():
    from telescope_amd import synthetic
    b = S.matrix('rowstats_1')
    raw = b.raw
    for off in (0, 333, (1 << 40) + 5):
        cnt, h32 = S.signature(raw, off)
        want = [0] * raw.shape[1]
        for i in range(0, raw.shape[0], 7):
            hr = S.row_hash(i + off)
            assert hr == int(synthetic.mix64(np.uint64(0x7715) ^ np.uint64(((i + off) * S.GOLDEN) & S.M64))) >> 32
            assert 0 <= hr <= S.M32
        for i in range(raw.shape[0]):
            hr = S.row_hash(i + off)
            for k in range(raw.indptr[i], raw.indptr[i + 1]):
                want[raw.indices[k]] = (want[raw.indices[k]] + S.entry_hash(hr, int(raw.data[k]))) & S.M32
        assert [int(x) for x in h32] == want
        assert np.array_equal(cnt, np.bincount(raw.indices, minlength=raw.shape[1]))


@pytest.mark.parametrize('name', NAMES)
def test_matrix_lands_in_its_variant(name):
    b = S.matrix(name)
    want_r, want_c = S.intended_lanes(name)
    assert want_r in (None, S.rowstats_lanes(b.raw)) and want_c in (None, S.colsig_lanes(b.raw)), (name, S.rowstats_lanes(b.raw), S.colsig_lanes(b.raw))
    lens = np.diff(b.raw.indptr)
    kind, _, arg = name.partition('_')
    if kind in ('rowstats', 'colsig'):
        G = 4 if arg == 'zero' else int(arg)
        if kind == 'rowstats':
            assert set(S.special_lengths(G)) <= set(lens.tolist())
        else:                                                           # exactly the 0.5 % that still picks G; G > 1: G / 2 would not do
            assert (lens > 16 * G).sum() == 5 and len(lens) == 1000 and lens.max() >= min(3 * 16 * G, 257)
            assert G == 1 or (lens > 8 * G).sum() > S.LONG_SHARE * len(lens)
        assert lens[-1] % 16 == 1 and len(b.behind) >= 2
        first = 0 if arg == 'zero' else S.BIG
        for r in b.behind:                                              # the marked code right behind a row of 1 mod 16 entries with small codes
            a, z = b.raw.indptr[r - 1], b.raw.indptr[r]
            assert (z - a) % 16 == 1 and b.raw.data[a:z].max() < S.SMALL and b.raw.data[z] == first
        assert int(b.raw.data.max()) == S.BIG
        assert bool((b.raw.data == 0).any()) == (arg == 'zero')
        # the twin cases: a pair, a triple, equal counts with one other score, equal counts with one other row
        cnt, _ = S.signature(b.raw)
        rep, _ = S.true_twins(b.raw)
        c = b.cols
        assert rep[c['pair'][1]] == c['pair'][0] and rep[c['triple'][1]] == rep[c['triple'][2]] == c['triple'][0]
        for k in ('score', 'row'):
            assert cnt[c[k][0]] == cnt[c[k][1]] > 0 and rep[c[k][0]] != rep[c[k][1]]
    if kind == 'window':
        K = int(arg)
        cnt, _ = S.signature(b.raw)
        rep, _ = S.true_twins(b.raw)
        for c in S.WINDOW_COLS:
            assert c >= K or cnt[c] > 0, (K, c)
        for t in (b.cols.get('pair'), b.cols.get('triple')):            # twins across a window boundary
            if t:
                assert all(rep[x] == t[0] for x in t)
        assert K == 18432 or any(len(set(x // S.SIG_WIN for x in t)) > 1 for t in (b.cols.get('pair'), b.cols.get('triple')) if t)


def test_shards_are_fair():
    b = S.matrix('rowstats_2')
    r = S.shard_cut(b)
    n = b.raw.shape[0]
    top, bottom = S.shard(b.raw, 0, r), S.shard(b.raw, r, n)
    assert r % 16 and top.nnz + bottom.nnz == b.raw.nnz
    c0, h0 = S.signature(top, 0)
    c1, h1 = S.signature(bottom, r)
    cnt, h32 = S.signature(b.raw)
    assert np.array_equal(c0 + c1, cnt) and np.array_equal((h0 + h1) & np.uint64(S.M32), h32)
    assert S.colliding_columns(top, 0) == [] and S.colliding_columns(bottom, r) == []
    p, q = b.cols['row']                                                # twins inside the upper shard only
    rep_top, rep_all = S.true_twins(top)[0], S.true_twins(b.raw)[0]
    assert rep_top[q] == rep_top[p] and rep_all[q] != rep_all[p] and c0[p] > 0 and c1[p] > 0


def test_table_past_the_range_of_the_levels():
    """the reference's side of the defect: on a table spanning 979 binades the split alone drops what is left after the last level — a
    column whose unique rows hold only the smallest scores comes out as exactly 0 against a positive sum —, and with the remainder
    kept every column is within (n_j + PIS_LEVELS) 2^-53 of the exact sum and 0 only where that is 0, in either order"""
    b = S.matrix('wide_table')
    assert S.table_is_fair(b.lut) and S.table_span(b.lut) > S.PIS_EXACT_SPAN
    p = S.Pisum0(b.raw, b.lut)
    assert not p.remainder_exceeds_q
    assert p.n[7] == 40 and p.exact[7] > 0 and p.emulated[7] == 0.0 and p.left[7] > 0            # the old split: a relative error of 1
    old, _ = p.worst(p.emulated, extra_terms=True)
    assert old > 1e10
    for reverse in (False, True):
        kept = p.kept(reverse)
        frac, j = p.worst(kept, extra_terms=True)
        assert frac <= 1.0, (reverse, j, frac)
        assert np.array_equal(kept == 0, ~p.positive)
    large = p.left == 0                                                 # columns whose unique rows the levels take whole: still exact
    assert large[500] and p.n[500] == 30 and np.array_equal(p.kept()[large], p.emulated[large])
    assert S.level_plan(np.array([0.0, math.ldexp(1.0, 1000)])) == []  # no levels where the top level's constant would overflow
    h = S.matrix('huge_table')
    assert S.table_is_fair(h.lut) and S.level_plan(h.lut) == [] and np.isfinite(math.fsum(h.lut[h.raw.data].tolist()))
    ph = S.Pisum0(h.raw, h.lut)
    assert not ph.emulated.any() and ph.worst(ph.kept(), extra_terms=True)[0] <= 1.0 and ph.worst(ph.kept(True), extra_terms=True)[0] <= 1.0
    assert len(S.level_plan(np.array([0.0, math.ldexp(1.0, -900)]))) < S.PIS_LEVELS
