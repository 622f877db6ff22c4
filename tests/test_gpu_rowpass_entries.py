"""`-m gpu`: everything the row pass (k_rowpass, telescope_amd/csrc/tsem_report.hip) hands out per stored entry — the posterior z
(tsem_export_z, tsem_rows_lookup, tl.lookup), the six reassign masks (tsem_rows_lookup, tl.reassign(...).tocsr()) and the
`--updated_sam` tag words (tsem_entry_tags, tl.entry_tag_tiles) — against tests/_rowpass_reference.py: an exact (long double)
reference, the reference implementation's own fp64 operator sequence (the oracle) and the host quantiser, tied down without a
GPU by tests/test_rowpass_reference.py.  Both sides always hold the SAME parameters (eng.set_params).

On ALL entries of every matrix, for the sources of z it is run with:
 1. |z - exact_z| <= bound(len) exact_z, bound(len) = (len + 3) 2^-53; pattern identical; rows of one or two stored entries
    bit-equal to the oracle's z (their sum is one addition);
 2. tag words: fields 0-15 and bit 17 bit-equal to tag_word(z as exported) — with 1, every word is pinned to the exact value
    within the bound;
 3. bit 16 and the masks: equal to `oracle.reassign(method) > 0` on every row, to the exact assignment on clear rows; `average` /
    `conf` values within 2 bound(len) of the exact ones;
 4. all six methods, `choose` with picks (indexed per tile row in the tag pass).

Every leg prints `ROWPASS ...` lines with the figures it asserts on (`pytest -s`); profiles/r09_rowpass_entries.txt keeps a run:
the largest z error seen is 0.88 of the bound, the file takes ~4 minutes, three quarters of them in test_rowpass_entries_at_size."""
import time

import numpy as np
import pytest
import scipy.sparse as sp

import _rowpass_reference as R
from conftest import Opts

pytestmark = pytest.mark.gpu
LD = R.LD
FIELDS = np.uint32(0x2FFFF)                       # MAPQ, XP and the z >= 0.2 bit: everything but the assigned bit
LAYOUTS = [{}, {'value_format': 1}, {'value_format': 2}, {'hot_split': 0}, {'drop_csr_indices': 1}, {'report_kernel': 0}]


def _dev(which):
    from telescope_amd import _lib
    return {R.CUR: _lib.Z_CUR, R.PREV: _lib.Z_PREV, R.INITIAL: _lib.Z_INITIAL, R.USER: _lib.Z_USER}[which]


def _say(fmt, *a):
    print('ROWPASS ' + fmt % a, flush=True)


def _engine(gpu_device, raw, lut, layout=None):
    """An engine holding `raw` with the caller's score table `lut` and a model set through the C ABI alone (tsem_rowstats ->
    tsem_set_model, the reference's priors)."""
    from telescope_amd import _lib
    eng = _lib.Engine(gpu_device)
    for key, v in (layout or {}).items():
        eng.set_option(key, v)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], lut)
    stats, pisum0, cnt, hsh = eng.rowstats()
    eng.set_model(stats, pisum0, cnt, hsh, 0, 200000)
    return eng


def _model(gpu_device, raw, lut, layout=None, em=True):
    """An engine holding `raw`, wrapped as a TelescopeLikelihood (from_engine: `lut` must be the model's own table, score_lut of the
    largest score) and laid out by one EM iteration — the blocked layout, the popularity ids and the dropped column ids exist only
    after it.  The wrapper is told its matrix (`_raw`, as the other engine-level tests do) and that its z is the CURRENT parameters'
    (`_z_which`: the caller sets them with eng.set_params afterwards)."""
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood
    eng = _lib.Engine(gpu_device)
    for key, v in (layout or {}).items():
        eng.set_option(key, v)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], lut)
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=1, em_epsilon=0.0))
    assert np.array_equal(np.asarray(lut), tl._lut), 'the model built its own score table: not the one the reference uses'
    tl._raw = raw
    if em and min(raw.shape) >= 8:
        tl.em()
    tl._z, tl._z_which = None, _lib.Z_CUR
    info = eng.layout_info()
    for key, v in (layout or {}).items():                           # the option was taken, not quietly replaced by the default layout
        if key == 'value_format':
            assert info['value_bytes'] == (2 if v == 2 else 8) and (v != 2 or info['fused'] == 1), (layout, info)
        if key == 'hot_split' and v == 0:
            assert info['hot_cols'] == 0, (layout, info)
    return eng, tl


def _tiles(n, rng):
    """arbitrary cuts of [0, n): empty tiles, one-row tiles, the rest random"""
    cuts = sorted(set([0, n] + list(rng.randint(0, n + 1, size=min(n, 6))) + ([1, 2] if n > 2 else [])))
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += [(a, a), (a, b)]
    return out


def _check_z(z, ref, label, what):
    """check 1 on a device z laid out on the stored entries (-1: not in z's pattern); returns the largest error / bound"""
    rid = R.row_ids(ref.indptr)
    assert z.shape == ref.inpat.shape and not np.any(np.isnan(z)), (label, what)
    assert np.array_equal(z != -1.0, ref.inpat), (label, what, 'pattern', np.flatnonzero((z != -1.0) != ref.inpat)[:5])
    zd = np.where(ref.inpat, z, 0.0)
    frac = R.error_fraction(zd, ref.z, ref.inpat, ref.indptr, per_entry=True)
    worst = int(np.argmax(frac)) if len(frac) else 0
    top = float(frac[worst]) if len(frac) else 0.0
    _say('%s %s: largest z error %.3f of bound(len) (row %d, %d entries)', label, what, top, rid[worst] if len(frac) else -1,
         ref.lens[rid[worst]] if len(frac) else 0)
    assert top <= 1.0, (label, what, rid[worst], ref.lens[rid[worst]], float(zd[worst]), float(ref.z[worst]))
    short = (ref.lens <= 2)[rid]
    bad = np.flatnonzero(short & (zd != ref.zn))
    assert len(bad) == 0, (label, what, 'rows of one or two entries', rid[bad[:5]], zd[bad[:5]], ref.zn[bad[:5]])
    return top, zd


def _check_mask(m, ref, method, label, what, parts=None):
    """check 3 on assignment values laid out on the stored entries"""
    o, e, clear = parts if parts is not None else ref.assigned(method)
    rid = R.row_ids(ref.indptr)
    bad = np.flatnonzero((m > 0) != (o > 0))
    assert len(bad) == 0, (label, what, method, 'differs from the oracle in rows', rid[bad[:5]], 'clear:', clear[rid[bad[:5]]])
    c = clear[rid]
    bad = np.flatnonzero(((m > 0) != (e > 0)) & c)
    assert len(bad) == 0, (label, what, method, 'differs from the exact assignment in clear rows', rid[bad[:5]])
    if method in ('average', 'conf'):
        lim = 2 * R.bound(ref.lens)[rid] * e
        bad = np.flatnonzero((np.abs(m.astype(LD) - e) > lim) & c)
        assert len(bad) == 0, (label, what, method, rid[bad[:5]], m[bad[:5]], e[bad[:5]])
    else:
        assert np.array_equal(m, o), (label, what, method, 'values')


def _check_words(w, zd, ref, method, label, what, parts):
    """checks 2 and 3 on the tag words of all stored entries"""
    from telescope_amd import bam_out
    o, e, clear = parts
    rid = R.row_ids(ref.indptr)
    assert w.dtype == np.uint32 and w.shape == zd.shape, (label, what, method)
    want = bam_out.tag_word(zd, np.zeros(len(zd)))
    bad = np.flatnonzero(((w & FIELDS) != want) | ((w >> np.uint32(18)) != 0))
    assert len(bad) == 0, (label, what, method, 'MAPQ / XP / 0.2 fields', rid[bad[:5]], [hex(int(x)) for x in w[bad[:5]]],
                           [hex(int(x)) for x in want[bad[:5]]], zd[bad[:5]])
    a = (w >> np.uint32(16) & np.uint32(1)).astype(bool)
    bad = np.flatnonzero(a != (o > 0))
    assert len(bad) == 0, (label, what, method, 'assigned bit differs from the oracle in rows', rid[bad[:5]], clear[rid[bad[:5]]])
    bad = np.flatnonzero((a != (e > 0)) & clear[rid])
    assert len(bad) == 0, (label, what, method, 'assigned bit differs from the exact assignment in clear rows', rid[bad[:5]])


def _sparse_picks(ref):
    rows = np.flatnonzero(ref.nbo > 1).astype(np.int32)             # (the rows the reference would draw for)
    return rows, ref.picks[rows].astype(np.int32)


def _redone(eng, call):
    """(what `call` returns, the growth of `near_tie_rows` over it): the rows ONE pass left to its FIX launch"""
    before = eng.layout_info()['near_tie_rows']
    out = call()
    return out, eng.layout_info()['near_tie_rows'] - before


def check_everything(eng, tl, ref, label, seed=0, tl_level=True, methods=R.METHODS, near_ties=False, min_clear=0.99):
    """Checks 1 - 4 of the module docstring on every stored entry.  Returns the largest z error as a fraction of the bound and, per
    (method, pass), the rows that ONE pass over the whole matrix sent through its FIX launch — the mask pass of rows_lookup and the
    one-tile tag pass (`near_tie_rows` read before and after that single call)."""
    from telescope_amd import bam_out
    from telescope_amd.likelihood import Assignment
    raw, which, thresh = ref.raw, _dev(ref.which), ref.thresh
    n = raw.shape[0]
    rid = R.row_ids(ref.indptr)
    rng = np.random.RandomState(seed)
    share = ref.clear_share()
    _say('%s: %d rows, %d entries, %.2f %% of the rows clear, %d rows with several best hits', label, n, raw.nnz, 100 * share,
         int((ref.nb > 1).sum()))
    if near_ties:
        assert share < 0.5, (label, share)
    else:
        assert share >= min_clear, (label, share)
    if ref.which == R.USER:
        eng.set_user_z(ref.user_z)
    # 1. z: the export, the compact look-up of all rows, and tl.lookup on a shuffled subset with repeats
    top, zd = _check_z(eng.export_z(which), ref, label, 'export_z')
    rows = np.arange(n, dtype=np.int32)
    z2, _ = eng.rows_lookup('exclude', thresh, which, rows, ref.indptr, want_mask=False)
    top = max(top, _check_z(z2, ref, label, 'rows_lookup')[0])
    sub = rng.randint(0, n, min(n, 5000) + 7).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(ref.lens[sub])]).astype(np.int64)
    pos = np.concatenate([np.arange(ref.indptr[r], ref.indptr[r + 1]) for r in sub]) if len(sub) else np.zeros(0, np.int64)
    z3, _ = eng.rows_lookup('exclude', thresh, which, sub, off, want_mask=False)
    assert np.array_equal(z3, z2[pos]), (label, 'rows_lookup of a shuffled list with repeats')
    ent = None
    if tl_level and raw.nnz:
        ent = ref.indptr[sub] + (rng.random_sample(len(sub)) * ref.lens[sub]).astype(np.int64)     # one stored entry of each listed row
    tab = bam_out.phred_table()
    passes = {}
    for method in methods:
        parts = ref.assigned(method)
        pk = ref.picks if method == 'choose' else None
        # 3. the masks of the compact look-up (all rows; picks by list position) and of tl.reassign(...).tocsr()
        (_, m), passes[(method, 'rows_lookup')] = _redone(eng, lambda: eng.rows_lookup(method, thresh, which, rows, ref.indptr, pk, want_z=False))
        _check_mask(m, ref, method, label, 'rows_lookup', parts)
        _, m3 = eng.rows_lookup(method, thresh, which, sub, off, None if pk is None else pk[sub], want_z=False)
        assert np.array_equal(m3, m[pos]), (label, method, 'rows_lookup of a shuffled list with repeats')
        # 2. + 3. the tag words over arbitrary cuts and over one tile
        tiles = _tiles(n, rng)
        got = [eng.entry_tags(method, thresh, which, r0, r1, tab, None if pk is None else pk[r0:r1],
                              n_out=ref.indptr[r1] - ref.indptr[r0]) for r0, r1 in tiles]
        _check_words(np.concatenate(got), zd, ref, method, label, 'entry_tags over %d cuts' % len(tiles), parts)
        whole, passes[(method, 'entry_tags')] = _redone(eng, lambda: eng.entry_tags(method, thresh, which, 0, n, tab, pk, n_out=raw.nnz))
        _check_words(whole, zd, ref, method, label, 'entry_tags, one tile', parts)
        if tl_level:
            a = Assignment(tl, method, thresh, which, _sparse_picks(ref) if method == 'choose' else None)
            _check_mask(R.align(a.tocsr(), raw).astype(np.float64), ref, method, label, 'tl.reassign(...).tocsr()', parts)
            words = 37 if raw.nnz <= 200000 else 100003            # (a tile costs two launches and three copies)
            t = list(tl.entry_tag_tiles(method, thresh, assignment=a, tile_bytes=4 * words))
            assert t[0][0] == 0 and t[-1][1] == n and all(u[1] == v[0] for u, v in zip(t, t[1:])), (label, method)
            _check_words(np.concatenate([u[2] for u in t]), zd, ref, method, label, 'tl.entry_tag_tiles, %d words' % words, parts)
            prob, val = tl.lookup(rid[ent], raw.indices[ent], method, thresh, assignment=a)
            assert np.array_equal(prob, zd[ent]) and np.array_equal(val.astype(np.float64), m[ent]), (label, method, 'tl.lookup')
    _say('%s: rows redone by the FIX launch of one pass over the matrix: %s', label,
         ', '.join('%s %s %d' % (k[0], k[1], v) for k, v in passes.items()))
    assert all(0 <= v <= n for v in passes.values()), passes
    if ref.which == R.USER:
        eng.set_user_z(None)
    return top, passes


# ---- (a) shapes ---------------------------------------------------------------------------------------------------------------------
SHAPE_NAMES = sorted(R.SHAPES)
CODES = LAYOUTS.index({'value_format': 2})
# Forcing the 2-byte entry format needs the fused EM kernel, which does not take these matrices (rows of thousands of entries, or
# no ambiguous row at all): tsem_set_model refuses the option by name and no row pass exists to check.  They are left out of the
# shapes x layouts product and held to that refusal below; every other shape MUST take the option (value_bytes == 2, _model).
REFUSED_UNDER_CODES = ('last_row_longest', 'len_1', 'len_5000', 'mixed', 'one_column', 'single_only')
SHAPE_LAYOUTS = [(name, layout) for name in SHAPE_NAMES for layout in range(len(LAYOUTS))
                 if not (layout == CODES and name in REFUSED_UNDER_CODES)]


@pytest.mark.parametrize('name', REFUSED_UNDER_CODES)
def test_forced_code_entries_are_refused_by_name(gpu_device, name):
    from telescope_amd import _lib
    raw, lut, _, _ = R.shape_case(name)
    with pytest.raises(_lib.EngineError, match='value_format=codes needs the fused kernel'):
        _model(gpu_device, raw, lut, LAYOUTS[CODES])


@pytest.mark.parametrize('name,layout', SHAPE_LAYOUTS)
def test_rowpass_entries_on_rows_of_every_shape(gpu_device, name, layout):
    """Row lengths 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 5000 alone and mixed; 1 row, 1 column, 300 000 rows (more than
    one sweep of the 8192 x 16-row grid); single-entry rows first / last / only; the last row the longest — under every layout the
    matrix can have (see REFUSED_UNDER_CODES).  The current z in all of them; under the default layout also the initial z and a
    caller's z with NaN holes."""
    raw, lut, pi, theta = R.shape_case(name)
    eng, tl = _model(gpu_device, raw, lut, LAYOUTS[layout])
    eng.set_params(pi, theta)
    label = 'a/%s/%s' % (name, LAYOUTS[layout] or 'default')
    top, _ = check_everything(eng, tl, R.Reference(raw, lut, pi, theta, seed=layout), label + '/cur', seed=layout)
    if layout == 0:
        t2, _ = check_everything(eng, tl, R.Reference(raw, lut, which=R.INITIAL, seed=1), label + '/initial', seed=1, tl_level=False)
        uz = R.user_z_of(raw, lut, pi, theta)
        t3, _ = check_everything(eng, tl, R.Reference(raw, lut, which=R.USER, user_z=uz, seed=2), label + '/user', seed=2, tl_level=False)
        top = max(top, t2, t3)
    _say('LEG a %s: %.3f of bound(len)', label, top)
    eng.close()


@pytest.mark.parametrize('name', ['mixed', 'last_row_longest', 'len_5000'])
def test_rowpass_entries_with_the_score_table_in_global_memory(gpu_device, name):
    """scores up to 5000: the table (5001 entries) does not fit the 2048 LDS slots, the row pass reads it from global memory and the
    PHRED table sits at the start of the LDS"""
    raw, lut, pi, theta = R.shape_case(name, 5000)
    assert len(lut) > 2048
    eng, tl = _model(gpu_device, raw, lut)
    eng.set_params(pi, theta)
    label = 'a/%s/table of %d' % (name, len(lut))
    top, _ = check_everything(eng, tl, R.Reference(raw, lut, pi, theta), label + '/cur')
    t2, _ = check_everything(eng, tl, R.Reference(raw, lut, which=R.INITIAL, seed=1), label + '/initial', seed=1, tl_level=False)
    _say('LEG a %s: %.3f of bound(len)', label, max(top, t2))
    eng.close()


def test_rowpass_entries_of_both_parameter_sets_after_em(gpu_device):
    """TSEM_Z_PREV and TSEM_Z_CUR after three EM iterations of the engine itself: the parameters are downloaded (get_params), so the
    reference holds the device's own numbers; `tl.z` is the previous set's z (the E-step before the last M-step)."""
    from telescope_amd import _lib
    raw, lut, _, _ = R.shape_case('mixed')
    eng, tl = _model(gpu_device, raw, lut, em=False)
    tl.max_iter = 3
    tl.em()
    assert tl._z_which == _lib.Z_PREV
    top = 0.0
    for which, code in ((R.PREV, _lib.Z_PREV), (R.CUR, _lib.Z_CUR)):
        pi, theta = eng.get_params(code)
        tl._z, tl._z_which = None, code
        t, _ = check_everything(eng, tl, R.Reference(raw, lut, pi, theta, which=which, seed=4), 'a/mixed/after em/' + which, seed=4)
        top = max(top, t)
    _say('LEG a a/mixed/after em: %.3f of bound(len)', top)
    eng.close()


# ---- (b) planted thresholds, bit-exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('table_len,part,parts', [(2048, 0, 2), (2048, 1, 2), (8192, 0, 1)])
def test_rowpass_entries_on_planted_thresholds(gpu_device, table_len, part, parts):
    """Two-entry rows (x, fl(1 - x)) with x + fl(1 - x) == 1.0 over a caller-supplied score table: z == x exactly, so every tag word
    is known bit for bit — x on every PHRED step, XP rounding tie, 0.2, conf_prob = 0.9, 0, 1 and their neighbours at +-1 and +-2
    ulp.  Through the initial z, through the current z with dyadic parameters, and as a caller's z with NaN holes; with the score
    table in LDS (2048 entries, in two halves) and in global memory (8192 entries, the planted values at its end)."""
    from telescope_amd import bam_out
    raw, lut, x = R.planted_case(table_len, part, parts)
    pi, theta = R.dyadic_parameters(raw.shape[1], np.random.RandomState(3))
    eng = _engine(gpu_device, raw, lut)                            # (a caller-supplied table: the engine alone, no model wrapper)
    eng.set_params(pi, theta)
    y = 1.0 - x
    uz = np.stack([x, np.where(np.arange(len(x)) % 5 == 4, np.nan, y)], axis=1).ravel()
    tab = bam_out.phred_table()
    for which, kw in ((R.INITIAL, {}), (R.CUR, dict(pi=pi, theta=theta)), (R.USER, dict(user_z=uz))):
        ref = R.Reference(raw, lut, which=which, thresh=0.9, **kw)
        want_z = np.where(np.isnan(uz), 0.0, uz) if which == R.USER else np.stack([x, y], axis=1).ravel()
        assert np.array_equal(ref.zn, want_z)
        if which == R.USER:
            eng.set_user_z(uz)
        z = eng.export_z(_dev(which))
        assert np.array_equal(np.where(z == -1.0, 0.0, z), want_z), (which, np.flatnonzero(np.where(z == -1.0, 0.0, z) != want_z)[:5])
        for method in R.METHODS:
            o = R.oracle_assigned(ref.om, raw, method, 0.9, which, ref.picks)
            want = bam_out.tag_word(ref.zn, o)                              # numpy's z, the oracle's assignment, the host quantiser
            got = eng.entry_tags(method, 0.9, _dev(which), 0, raw.shape[0], tab, ref.picks if method == 'choose' else None, n_out=raw.nnz)
            bad = np.flatnonzero(got != want)
            assert len(bad) == 0, (which, method, want_z[bad[:5]], [hex(int(v)) for v in got[bad[:5]]], [hex(int(v)) for v in want[bad[:5]]])
        top, _ = check_everything(eng, None, ref, 'b/table of %d, part %d/%s' % (table_len, part, which), tl_level=False)
        _say('LEG b table of %d, part %d, %s: %.3f of bound(len); %d planted rows, every word equal', table_len, part, which, top, len(x))
    eng.close()


# ---- (c) dead and dying columns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('report_kernel', [1, 0])
@pytest.mark.parametrize('kind', R.DEAD_KINDS)
def test_rowpass_entries_with_dead_columns(gpu_device, kind, report_kernel):
    """pi or theta zero on a fifth of the columns (rows that lose some, all but one, or all of their entries, in both paths of the
    pass), subnormal and underflowing pi * theta, stored scores of 0 with and without lut[0] == 0: the current z, and the same z
    handed back as a caller's z with NaN outside the pattern."""
    raw, lut, pi, theta = R.dead_column_case(kind)
    own = kind != 'zero_score'                                      # (lut[0] > 0 is a caller's table: the engine alone then)
    eng, tl = _model(gpu_device, raw, lut, {'report_kernel': report_kernel}) if own else \
        (_engine(gpu_device, raw, lut, {'report_kernel': report_kernel}), None)
    eng.set_params(pi, theta)
    label = 'c/%s/report_kernel %d' % (kind, report_kernel)
    ref = R.Reference(raw, lut, pi, theta)
    assert np.any(~ref.inpat) or kind == 'zero_score'
    top, _ = check_everything(eng, tl, ref, label + '/cur', tl_level=own)
    uz = np.where(ref.inpat, ref.zn, np.nan)
    t2, _ = check_everything(eng, tl, R.Reference(raw, lut, which=R.USER, user_z=uz, seed=2), label + '/user', seed=2, tl_level=False)
    _say('LEG c %s: %.3f of bound(len)', label, max(top, t2))
    eng.close()


# ---- (d) near-ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed,kw', R.NEAR_TIE_CASES)
def test_rowpass_entries_on_near_ties(gpu_device, seed, kw):
    """The five matrices of test_gpu_round6 (columns in pairs whose pi * theta are one to three ulp apart): bit 16 and the masks equal
    the oracle's on EVERY row, z stays within the bound, and EVERY pass sends rows through its FIX launch: `near_tie_rows` is read
    around each single pass over the matrix (the mask pass of rows_lookup, the one-tile tag pass), for each method."""
    from telescope_amd.likelihood import score_lut
    raw, pi, theta = R.near_tie_matrix(seed, **kw)
    n = raw.shape[0]
    lut = score_lut(int(raw.data.max()))
    eng, tl = _model(gpu_device, raw, lut)
    eng.set_params(pi, theta)
    ref = R.Reference(raw, lut, pi, theta, seed=seed)
    top, passes = check_everything(eng, tl, ref, 'd/seed %d' % seed, seed=seed, near_ties=True)
    assert len(passes) == 12 and all(0 < v <= n for v in passes.values()), passes
    _say('LEG d seed %d (%d rows, %.2f %% clear): %.3f of bound(len); rows redone by ONE pass: rows_lookup %s, entry_tags %s', seed, n,
         100 * ref.clear_share(), top, {m: passes[(m, 'rows_lookup')] for m in R.METHODS}, {m: passes[(m, 'entry_tags')] for m in R.METHODS})
    # `conf` at a threshold that IS the largest z of many rows (it compares with >=), as test_gpu_round6 has it
    th = R.z_value_threshold(ref)
    ref2 = R.Reference(raw, lut, pi, theta, thresh=th, seed=seed)
    on = int(np.sum(ref2.zn == th))
    t, p2 = check_everything(eng, tl, ref2, 'd/seed %d/conf at %r' % (seed, th), seed=seed, methods=('conf',), near_ties=True)
    _say('LEG d seed %d, conf at a threshold %d entries sit on: %.3f of bound(len); rows redone by ONE pass: rows_lookup %d, entry_tags %d',
         seed, on, t, p2[('conf', 'rows_lookup')], p2[('conf', 'entry_tags')])
    assert on > 0 and all(0 < v <= n for v in p2.values()), p2
    eng.close()


# ---- (e) size -----------------------------------------------------------------------------------------------------------------------
def _generated(gpu_device, rows, cols, d, uniq, iters):
    from telescope_amd import _lib, synthetic
    from telescope_amd.likelihood import TelescopeLikelihood
    eng = _lib.Engine(gpu_device)
    eng.generate(0, rows, cols, synthetic.poisson_cdf_u32(d), 42, synthetic.DIST_CODE['zipf'], uniq)
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=iters, em_epsilon=0.0))
    tl.em()
    return eng, tl


def test_rowpass_entries_at_size(gpu_device):
    """The device generator at 2 M x 30 k x ~20 (5 % unique rows), five EM iterations, the parameters downloaded and set again so
    that both sides hold the same numbers: every check on all ~4e7 entries — the tag pass in one tile (125 000 workgroups' worth of
    rows, far beyond the grid of 8192: the grid-stride loop), over random cuts, and in a million tiles of 37 words."""
    from telescope_amd import _lib, synthetic
    from telescope_amd.likelihood import Assignment
    t0 = time.time()
    n, k = 2_000_000, 30_000
    eng, tl = _generated(gpu_device, n, k, 20, 0.05, 5)
    pi, theta = eng.get_params(_lib.Z_CUR)
    eng.set_params(pi, theta)
    tl._z, tl._z_which = None, _lib.Z_CUR
    ip, ix, rw = synthetic.generate(n, k, 20, seed=42, dist='zipf', uniq_frac=0.05)
    raw = sp.csr_matrix((rw, ix, ip), shape=(n, k))
    tl._raw = raw
    assert eng.dims() == (n, k, raw.nnz) and n // 16 > 8192
    ref = R.Reference(raw, tl._lut, pi, theta)
    t1 = time.time()
    top, _ = check_everything(eng, tl, ref, 'e/2M')
    # tiles of 37 words over the whole matrix (a million tiles), `choose` with its picks cut per tile
    tt = time.time()
    a = Assignment(tl, 'choose', 0.9, _lib.Z_CUR, _sparse_picks(ref))
    words, r_end = [], 0
    for r0, r1, w in tl.entry_tag_tiles('choose', 0.9, assignment=a, tile_bytes=4 * 37):
        assert r0 == r_end and len(w) == ip[r1] - ip[r0] and (len(w) <= 37 or r1 == r0 + 1)
        words.append(w); r_end = r1
    assert r_end == n
    per_tile = (time.time() - tt) / len(words)
    z = eng.export_z(_lib.Z_CUR)
    _check_words(np.concatenate(words), np.where(z == -1.0, 0.0, z), ref, 'choose', 'e/2M', 'tl.entry_tag_tiles, 37 words', ref.assigned('choose'))
    _say('LEG e 2M x 30k: %.3f of bound(len) over %d entries; %d tiles of 37 words at %.2f ms each; reference %.0f s, checks %.0f s',
         top, raw.nnz, len(words), 1e3 * per_tile, t1 - t0, time.time() - t1)
    eng.close()


def test_rowpass_entries_beyond_2_31_entries(gpu_device):
    """The matrix of test_more_than_2_31_entries_on_one_gpu (60 M x 30 k x ~40, 2.4e9 stored entries): the last 200 000 rows — the tag
    pass writes them with `tag_base` > 2^31 — against reference rows from the host generator, parameters downloaded once."""
    from telescope_amd import _lib, bam_out, synthetic
    t0 = time.time()
    n, k, tail = 60_000_000, 30_000, 200_000
    eng, tl = _generated(gpu_device, n, k, 40, 0.0, 3)
    assert eng.dims()[2] > 2 ** 31
    pi, theta = eng.get_params(_lib.Z_CUR)
    ip, ix, rw = synthetic.generate(n, k, 40, seed=42, dist='zipf', row_begin=n - tail, row_end=n)
    raw = sp.csr_matrix((rw, ix, ip), shape=(tail, k))
    ref = R.Reference(raw, tl._lut, pi, theta)
    _say('e/60M: %d rows, %d entries, %.2f %% of the rows clear', tail, raw.nnz, 100 * ref.clear_share())
    assert ref.clear_share() >= 0.99
    rows = np.arange(n - tail, n, dtype=np.int32)
    ipd = tl._eng_indptr()
    base = int(ipd[n - tail])
    assert base > 2 ** 31 and np.array_equal(ipd[n - tail:] - base, ip)
    z, _ = eng.rows_lookup('exclude', 0.9, _lib.Z_CUR, rows, ip, want_mask=False)
    top, zd = _check_z(z, ref, 'e/60M', 'rows_lookup')
    tab = bam_out.phred_table()
    rng = np.random.RandomState(1)
    for method in R.METHODS:
        parts = ref.assigned(method)
        pk = ref.picks if method == 'choose' else None
        _, m = eng.rows_lookup(method, 0.9, _lib.Z_CUR, rows, ip, pk, want_z=False)
        _check_mask(m, ref, method, 'e/60M', 'rows_lookup', parts)
        got = []
        for r0, r1 in _tiles(tail, rng) + [(0, tail)]:
            got.append(eng.entry_tags(method, 0.9, _lib.Z_CUR, n - tail + r0, n - tail + r1, tab, None if pk is None else pk[r0:r1],
                                      n_out=ip[r1] - ip[r0]))
        _check_words(np.concatenate(got[:-1]), zd, ref, method, 'e/60M', 'entry_tags over cuts', parts)
        _check_words(got[-1], zd, ref, method, 'e/60M', 'entry_tags, one tile', parts)
    eng.entry_tags_end()
    _say('LEG e 60M x 30k, last %d rows (tag_base %d): %.3f of bound(len) over %d entries; %.0f s', tail, base, top, raw.nnz, time.time() - t0)
    eng.close()
