"""`-m gpu`: what the set-up unit hands to every later pass — tsem_rowstats and tsem_set_model of telescope_amd/csrc/tsem_setup.hip:
k_rowstats<G> in its five instantiations, k_pisum_finish, k_colsig<G> in its five, the window sweep over K, the twin search, the
counts behind the shortcuts of tsem_reassign — against tests/_setup_reference.py, a plain host reference in numpy, math.fsum and
Python integers whose inputs tests/test_setup_reference.py shows to be fair without a GPU.  The C ABI through _lib.Engine only.

What every leg asserts (the numbers in the `SETUP ...` lines, `pytest -s`; an error is printed as a fraction of its bound):
 1. rows: Y and w of row_info bit-equal on every row, max_score() the host's;
 2. sums: stats3[2] exact, stats3[0] and stats3[1] within (N - 1) 2^-53 relative of math.fsum — any order of N non-negative additions;
 3. pisum0: bit-equal to the emulated level split, within (PIS_LEVELS - 1) 2^-53 of the exact sum, exactly 0 where no unique row has a
    positive score, bit-equal on a second engine with another `block_rows` and on a second call;
 4. signatures: cnt the host's counts, hsh & 0xFFFFFFFF the modelled hash (the high half is not a function of the matrix, see the
    reference), E.twin_representatives(cnt, hsh) the true classes, layout_info()['twin_cols'] the true number of twin columns;
 5. layout_info N_amb, N_uni, nnz_amb the host's; reassign('unique') and reassign('all', initial) the host's counts with option
    "report_shortcuts" 1 and 0 (a matrix that stores a 0 gives the row pass's numbers, not the entry counts);
 6. layout_info()['rowstats_lanes'] / ['colsig_lanes']: the k_rowstats<G> / k_colsig<G> the matrix was built for ran.
The shard leg adds the signatures of two engines with row offsets 0 and r (r not a multiple of 16) with wrap-around; the last leg
loads a table PAST the range of the levels (include/telescope_em.h, tsem_rowstats) and asserts the wider bound and the zero pattern.
Not covered: a level sum of 2^26 pieces (67M unique rows in one column).  profiles/r16_setup_products.txt keeps a run."""
import numpy as np
import pytest

import _em_pass_reference as E
import _setup_reference as S

pytestmark = pytest.mark.gpu
PRIORS = (0, 200000)
M32 = np.uint64(S.M32)
_refs = {}
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


def _say(fmt, *a):
    print('SETUP ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _engine(gpu_device):
    """an _lib.Engine that remembers a HIP error (TSEM_ERR_HIP, TSEM_ERR_TIMEOUT) for the fixture above"""
    from telescope_amd import _lib

    class Engine(_lib.Engine):
        def _ck(self, rc):
            if rc in (-2, -4):
                _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
            _lib.Engine._ck(self, rc)
    return Engine(gpu_device)


class Ref(object):
    """the host's side of one matrix, computed once"""

    def __init__(self, raw, lut, row_offset=0):
        self.raw, self.lut = raw, lut
        self.Y, self.code, self.w = S.row_outputs(raw, lut)
        self.stats = S.stats3(raw, lut)
        self.pis = S.Pisum0(raw, lut)
        self.cnt, self.h32 = S.signature(raw, row_offset)
        self.rep, self.n_twin = S.true_twins(raw)
        self.counts = S.Counts(raw, lut)
        self.lanes = (S.rowstats_lanes(raw), S.colsig_lanes(raw))


def _ref(name):
    if name not in _refs:
        b = S.matrix(name)
        _refs[name] = Ref(b.raw, b.lut)
    return _refs[name]


class Setup(object):
    """an engine holding `raw` and `lut`, and what tsem_rowstats gave; model=True: tsem_set_model with the reference's priors"""

    def __init__(self, gpu_device, raw, lut, options=(), model=True):
        self.eng = eng = _engine(gpu_device)
        for key, v in options:
            eng.set_option(key, v)
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], lut)
        self.max_score = eng.max_score()
        self.rowstats()
        self.Y, self.w = eng.row_info()
        if model:
            eng.set_model(self.stats, self.pisum0, self.cnt, self.hsh, *PRIORS)
        self.info = eng.layout_info()

    def rowstats(self):
        self.stats, self.pisum0, self.cnt, self.hsh = self.eng.rowstats()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_rows_and_sums(m, ref, label):
    """checks 1 and 2; returns the fractions of W_tot and W_amb"""
    assert np.array_equal(m.Y, ref.Y), (label, 'Y', np.flatnonzero(m.Y != ref.Y)[:5])
    bad = np.flatnonzero(_bits(m.w) != _bits(ref.w))
    assert len(bad) == 0, (label, 'w differs in rows', bad[:5], m.w[bad[:5]], ref.w[bad[:5]], 'lengths', np.diff(ref.raw.indptr)[bad[:5]])
    assert m.max_score == int(ref.raw.data.max()), (label, m.max_score)
    n = ref.raw.shape[0]
    f_tot = S.sum_fraction(m.stats[0], ref.stats[0], n)
    f_amb = S.sum_fraction(m.stats[1], ref.stats[1], n)
    _say('%s: W_tot %.4f, W_amb %.4f of (N - 1) 2^-53 (N = %d); w_max %r', label, f_tot, f_amb, n, float(m.stats[2]))
    assert m.stats[2] == ref.stats[2], (label, 'w_max', m.stats[2], ref.stats[2])
    assert f_tot <= 1.0 and f_amb <= 1.0, (label, 'W_tot, W_amb', m.stats, ref.stats, f_tot, f_amb)
    return f_tot, f_amb


def _check_pisum0(m, ref, label):
    """check 3 on one set of outputs, inside the levels' range; returns the fraction"""
    p = ref.pis
    frac, j = p.worst(m.pisum0)
    bad = np.flatnonzero(_bits(m.pisum0) != _bits(p.emulated))
    zero_bad = np.flatnonzero((m.pisum0 == 0) != ~p.positive)
    _say('%s: pisum0 %.4f of (PIS_LEVELS - 1) 2^-53 (column %d, %d unique rows); %d columns differ from the emulation; %d of %d '
         'columns with unique rows differ from fsum', label, frac, j, p.n[j] if j >= 0 else 0, len(bad),
         int((m.pisum0 != p.exact).sum()), int((p.n > 0).sum()))
    assert len(bad) == 0, (label, 'pisum0 differs from the emulated split in columns', bad[:5], m.pisum0[bad[:5]], p.emulated[bad[:5]])
    assert frac <= 1.0, (label, 'pisum0', j, frac)
    assert len(zero_bad) == 0, (label, 'zero pattern of pisum0', zero_bad[:5])
    return frac


def _check_signature(cnt, hsh, ref, label, want_rep=None):
    """check 4 without the model: counts, the low half of the hash, the classes"""
    bad = np.flatnonzero(cnt != ref.cnt)
    assert len(bad) == 0, (label, 'entry counts differ in columns', bad[:5], cnt[bad[:5]], ref.cnt[bad[:5]])
    bad = np.flatnonzero((hsh & M32) != ref.h32)
    assert len(bad) == 0, (label, 'hash (low 32 bits) differs in columns', bad[:5], hsh[bad[:5]] & M32, ref.h32[bad[:5]])
    rep = E.twin_representatives(cnt, hsh)
    want_rep = ref.rep if want_rep is None else want_rep
    bad = np.flatnonzero(rep != want_rep)
    assert len(bad) == 0, (label, 'twin classes differ in columns', bad[:5], rep[bad[:5]], want_rep[bad[:5]])
    return rep


def _check_lanes(m, ref, name, label):
    """check 6"""
    got = (m.info['rowstats_lanes'], m.info['colsig_lanes'])
    want_r, want_c = S.intended_lanes(name)
    _say('%s: k_rowstats<%d>, k_colsig<%d>', label, got[0], got[1])
    assert got == ref.lanes, (label, 'lanes per row', got, ref.lanes)
    assert want_r in (None, got[0]) and want_c in (None, got[1]), (label, got, want_r, want_c)


def _check_counts(m, ref, label):
    """check 5"""
    from telescope_amd._lib import Z_INITIAL
    c, i = ref.counts, m.info
    assert (i['N_amb'], i['N_uni'], i['nnz_amb']) == (c.N_amb, c.N_uni, c.nnz_amb), (label, i, c.N_amb, c.N_uni, c.nnz_amb)
    assert i['twin_cols'] == ref.n_twin, (label, 'twin columns', i['twin_cols'], ref.n_twin)
    want_all = c.positive_entries if c.has_zero else c.entries
    for shortcuts in (1, 0):
        m.eng.set_option('report_shortcuts', shortcuts)
        uni, _ = m.eng.reassign('unique', 0.9, Z_INITIAL)
        al, _ = m.eng.reassign('all', 0.9, Z_INITIAL)
        bad = np.flatnonzero(uni != c.unique)
        assert len(bad) == 0, (label, 'unique, report_shortcuts %d' % shortcuts, bad[:5], uni[bad[:5]], c.unique[bad[:5]])
        bad = np.flatnonzero(al != want_all)
        assert len(bad) == 0, (label, 'all (initial), report_shortcuts %d' % shortcuts, bad[:5], al[bad[:5]], want_all[bad[:5]])
    m.eng.set_option('report_shortcuts', 1)
    _say('%s: N_amb %d, N_uni %d, nnz_amb %d, %d twin columns, unique %d, all %d%s', label, c.N_amb, c.N_uni, c.nnz_amb, ref.n_twin,
         int(c.unique.sum()), int(want_all.sum()), ' (a stored 0: the row pass, %d entries)' % int(c.entries.sum()) if c.has_zero else '')


@pytest.mark.parametrize('name', S.MATRICES)
def test_setup_products(gpu_device, name):
    """checks 1 - 6 on the matrices of _setup_reference: one per k_rowstats<G> (every special length, the largest code — in
    rowstats_zero a stored 0 — first behind a row of 1 mod 16 entries, the last row ending on such a length), one per k_colsig<G>
    (exactly the 0.5 % of longer rows that still picks G), K on and around the window boundaries of k_colsig, and a column of 20 000
    unique rows with scores from both ends of score_lut(65535)"""
    ref = _ref(name)
    m = Setup(gpu_device, ref.raw, ref.lut)
    _check_lanes(m, ref, name, name)
    _check_rows_and_sums(m, ref, name)
    _check_pisum0(m, ref, name)
    _check_signature(m.cnt, m.hsh, ref, name)
    _check_counts(m, ref, name)
    if ref.counts.has_zero:
        assert not np.array_equal(ref.counts.positive_entries, ref.counts.entries)
    # order-independence: another engine with another `block_rows`, two calls
    m2 = Setup(gpu_device, ref.raw, ref.lut, options=(('block_rows', 64 if m.info['R'] != 64 else 128),), model=False)
    first = m2.pisum0.copy()
    m2.rowstats()
    for label, got in (('second engine', first), ('second call', m2.pisum0)):
        bad = np.flatnonzero(_bits(got) != _bits(m.pisum0))
        assert len(bad) == 0, (name, label, 'pisum0 differs in columns', bad[:5])
    _check_signature(m2.cnt, m2.hsh, ref, name + '/second call')
    assert m2.stats[2] == ref.stats[2] and S.sum_fraction(m2.stats[0], ref.stats[0], ref.raw.shape[0]) <= 1.0
    m.eng.close()
    m2.eng.close()


def test_sharded_signatures_add_up(gpu_device):
    """two engines hold the rows [0, r) and [r, N) of rowstats_2 with row offsets 0 and r, r not a multiple of 16: the wrap-around u64
    sums of their (cnt, hsh) have the whole matrix's counts, low hash halves and classes; the pair of columns that are twins inside
    the upper shard only is classed there and not in the sum; every shard's own rows, sums and pisum0 hold too"""
    b = S.matrix('rowstats_2')
    whole = _ref('rowstats_2')
    r, n = S.shard_cut(b), b.raw.shape[0]
    cnt, hsh = np.zeros(b.raw.shape[1], np.uint64), np.zeros(b.raw.shape[1], np.uint64)
    pis = np.zeros(b.raw.shape[1])
    p, q = b.cols['row']
    for a, z in ((0, r), (r, n)):
        part = S.shard(b.raw, a, z)
        ref = Ref(part, b.lut, row_offset=a)
        m = Setup(gpu_device, part, b.lut, options=(('row_offset', a),))
        label = 'rows [%d, %d)' % (a, z)
        _check_rows_and_sums(m, ref, label)
        _check_pisum0(m, ref, label)
        rep = _check_signature(m.cnt, m.hsh, ref, label)
        _check_counts(m, ref, label)
        assert m.info['rowstats_lanes'] == ref.lanes[0] and m.info['colsig_lanes'] == ref.lanes[1], (label, m.info)
        if a == 0:
            assert rep[q] == p, (label, 'the twins of this shard', rep[p], rep[q])
        with np.errstate(over='ignore'):
            cnt, hsh = cnt + m.cnt, hsh + m.hsh
        pis = pis + m.pisum0
        m.eng.close()
    rep = _check_signature(cnt, hsh, whole, 'the shards added')
    assert rep[q] != rep[p]
    # (two exact sums added: within one more rounding of the whole matrix's exact sum)
    frac = max(whole.pis.fraction(pis, j, S.PIS_LEVELS) for j in np.flatnonzero(whole.pis.n))
    _say('shards cut at row %d: counts, hashes and %d twin columns add up; pisum0 of the two added %.4f of PIS_LEVELS 2^-53', r, whole.n_twin, frac)
    assert frac <= 1.0


@pytest.mark.parametrize('name', ('wide_table', 'huge_table'))
def test_table_past_the_range_of_the_levels(gpu_device, name):
    """a caller's table spanning 979 binades (fair: finite, non-negative, non-decreasing): whatever the levels leave of a Q is kept —
    pisum0[j] within (n_j + PIS_LEVELS) 2^-53 relative of the exact sum, 0 only where the exact sum is 0, and still bit-equal to the
    emulation where the levels take a column's rows whole.  (Before the remainder was kept, column 7 — 40 unique rows with the three
    smallest scores — came out as exactly 0, as did every other column's share below 2^226.)  huge_table: the last entry is past
    2^997, where the top level's rounding constant would overflow — no levels at all, every Q is added as a remainder."""
    b = S.matrix(name)
    ref = Ref(b.raw, b.lut)
    m = Setup(gpu_device, b.raw, b.lut, model=name == 'wide_table')
    _check_rows_and_sums(m, ref, name)
    _check_signature(m.cnt, m.hsh, ref, name)
    if name == 'wide_table':
        _check_counts(m, ref, name)
    p = ref.pis
    frac, j = p.worst(m.pisum0, extra_terms=True)
    zero_bad = np.flatnonzero((m.pisum0 == 0) != ~p.positive)
    whole = p.left == 0
    _say(name + ': pisum0 %.4f of (n_j + PIS_LEVELS) 2^-53 (column %d, %d unique rows); column 7: %r against %r; %d columns zero '
         'against a positive sum; %d columns taken whole by the levels', frac, j, p.n[j] if j >= 0 else 0, float(m.pisum0[7]),
         float(p.exact[7]), len(zero_bad), int((whole & (p.n > 0)).sum()))
    assert len(zero_bad) == 0, ('zero pattern of pisum0', zero_bad[:5], m.pisum0[zero_bad[:5]], p.exact[zero_bad[:5]])
    assert frac <= 1.0, ('pisum0', j, frac, float(m.pisum0[j]), float(p.exact[j]))
    assert np.array_equal(_bits(m.pisum0[whole]), _bits(p.emulated[whole]))
    m.eng.close()
