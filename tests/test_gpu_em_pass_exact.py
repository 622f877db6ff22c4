"""`-m gpu`: ONE EM pass, ONE log-likelihood pass and ONE parameter update of every rung of the ladder — the fused kernel
k_em_fused<P, MODE, FMT, GEO> with every team size, both entry formats and its geometries, the split layout, the two-pass kernels,
the CSR row passes, option "reproducible", the carried lnl — against tests/_em_pass_reference.py: an exact (long double) reference
with rounding bounds that are functions of counts, tied down without a GPU by tests/test_em_pass_reference.py.  Both sides always
hold the SAME parameters (eng.set_params): parameters spread over hundreds of decades, exact zeros, subnormal products, rows whose
every column is dead — states a run from pi = theta = 1 / K never visits.

What every leg checks, per parameter set (the numbers in the messages below):
 1. em_pass -> red: |red_j - exact_j| <= bound_j exact_j on every column, exact zeros exactly 0, red[K] == red[K+1] == 0, no NaN;
 2. lnl_pass (previous = current: set_params twice) against exact_lnl within its limit, for every form of the pass
    (fused_dbg 8192 / 16384 / 32768 and unforced);
 3. em_update: get_params(Z_CUR) equals the closed forms (model.py:733-740, in the reference's order: (thetasum + prior) / den;
    pisum0 + thetasum, + prior, / den) evaluated in fp64 on the device's own red, bit for bit — twins take their representative's
    sum where k_update's 1e-12 rule applies —, get_params(Z_PREV) equals what was set, diff_est within K 2^-53 sum|pi_hat - pi|;
 4. without another set_params: em_pass again (check 1 on the device's Z_CUR) and lnl_pass (check 2 on Z_PREV / Z_CUR) — a stale
    ctab, ctab_prev or hot-column copy fails here.
Every leg asserts from layout_info that the layout it forced was built, and prints `EMPASS ...` lines with the figures it asserts on
(`pytest -s`); profiles/r15_em_pass_exact.txt keeps a run."""
import numpy as np
import pytest

import _em_pass_reference as E

pytestmark = pytest.mark.gpu
LD = E.LD
PRIORS = (0, 200000)
SETS = ('uniform', 'decades', 'dying', 'dead_rows', 'subnormal')
FORMS = (0, 8192, 16384, 32768)
FZ_NS, FZ_XS = 6, 8                               # tsem_fused.h: register sets, exchange slots per team
_refs = {}
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


def _say(fmt, *a):
    print('EMPASS ' + fmt % a, flush=True)


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


@pytest.fixture(scope='module')
def cu_count(gpu_device):
    import torch
    return int(torch.cuda.get_device_properties(gpu_device).multi_processor_count)


def _ref(mkey, raw, pname):
    """the shared reference of (matrix, parameter set) with previous = current, computed once"""
    key = (mkey, pname)
    if key not in _refs:
        pi, theta = E.parameter_set(pname, raw)
        _refs[key] = E.PassReference(raw, E.lut(raw), pi, theta)
        assert _refs[key].fair == [], (key, _refs[key].fair)
    return _refs[key]


class Model(object):
    """An engine holding `raw` with its model set through the C ABI alone (tsem_rowstats -> tsem_set_model, the reference's priors),
    and what the update check needs of it: the stats, pisum0 as the device holds it (twins merged by tsem_set_model's 1e-12 rule)
    and the twin representatives."""

    def __init__(self, gpu_device, raw, options=(), lut=None):
        self.raw, self.lut, self.K = raw, E.lut(raw) if lut is None else lut, raw.shape[1]
        self.eng = eng = _engine(gpu_device)
        for key, v in options:
            eng.set_option(key, v)
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), self.K, self.lut)
        eng.max_score()                                             # (as the Python host does: the lnl pass's choice of form needs the range of the stored scores)
        self.stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(self.stats, pisum0, cnt, hsh, *PRIORS)
        self.rep = E.twin_representatives(cnt, hsh)
        self.pisum0 = E.twin_rule(pisum0, self.rep)[0]
        self.info = eng.layout_info()

    def path(self):
        i = self.info
        if i['split'] == 1:
            return E.SPLIT, 0
        if i['fused'] == 1 and i['nb'] > 0:
            return E.FUSED, int(i['P'])
        return E.UNTAGGED, 0


def _check_pass(m, ref, label, limit_of=None):
    """check 1; returns the largest error as a fraction of its bound"""
    m.eng.em_pass()
    return _check_red(m, ref, m.eng.read_reduce(0, m.K + 2), label, limit_of)


def _check_red(m, ref, red, label, limit_of=None, slots=True):
    """check 1 on a reduce buffer that is already read (an EM pass the caller ran, in a chunk for instance).  slots=False: the caller
    has read the buffer where slots K and K + 1 hold log-likelihoods (after a chunk's flush) and checks the time-out another way"""
    path, P = m.path()
    assert not np.any(np.isnan(red)), (label, 'NaN in the reduce buffer', np.flatnonzero(np.isnan(red))[:5])
    if slots:
        assert red[m.K] == 0.0 and red[m.K + 1] == 0.0, (label, 'time-out word / carried value', red[m.K:])
    limit = None if limit_of is None else limit_of(ref, P)
    frac, j = E.colsum_fraction(red[:m.K], ref.sums, ref.cnt, ref.lenmax, ref.gradual, path, P, limit=limit)
    zero = (ref.sums == 0) & (ref.gradual == 0)
    bad = np.flatnonzero(zero & (red[:m.K] != 0))
    if len(bad) or frac > 1.0:
        info = m.eng.layout_info()
        _say('%s FAILS: column %d (%d entries, longest row %d): %r against %r, %.4g of the bound; %d columns not 0 that are exactly 0 %s; '
             'reproducible %d, %d repeats', label, j, ref.cnt[j], ref.lenmax[j], float(red[j]), float(ref.sums[j]), frac, len(bad), bad[:5], info['reproducible'], info['bin_repeats'])
    assert len(bad) == 0, (label, 'columns that are exactly 0', bad[:5], red[bad[:5]])
    assert frac <= 1.0, (label, 'column', j, 'entries', int(ref.cnt[j]), 'longest row', int(ref.lenmax[j]), float(red[j]), float(ref.sums[j]), frac)
    return frac, red


def _check_lnl(m, ref, label):
    """check 2 for the form that is set; returns |lnl - exact| as a fraction of its limit"""
    _, P = m.path()
    m.eng.lnl_pass()
    lnl = float(m.eng.read_reduce(m.K, 1)[0])
    assert np.isfinite(lnl), (label, lnl)
    frac = float(abs(LD(lnl) - ref.lnl) / ref.lnl_limit_P(P))
    if frac > 1.0:
        _say('%s FAILS: lnl %r against %r, %.4g of its limit %.3g', label, lnl, float(ref.lnl), frac, float(ref.lnl_limit_P(P)))
    assert frac <= 1.0, (label, 'lnl', lnl, float(ref.lnl), frac)
    return frac


def _check_update(m, red, pi_set, theta_set, label, diff=None):
    """check 3; returns (|diff_est - exact| as a fraction of its bound, the new parameters, how many twins took their representative's sum).
    diff: the diff_est of an update the caller has run already (a chunk's); None: em_update runs here"""
    from telescope_amd._lib import Z_CUR, Z_PREV
    if diff is None:
        diff = m.eng.em_update()
    pi_c, th_c = m.eng.get_params(Z_CUR)
    pi_p, th_p = m.eng.get_params(Z_PREV)
    assert np.array_equal(pi_p.view(np.uint64), pi_set.view(np.uint64)) and np.array_equal(th_p.view(np.uint64), theta_set.view(np.uint64)), (label, 'Z_PREV')
    ts, took = E.twin_rule(red[:m.K], m.rep)
    pi_e, th_e, diff_e = E.exact_update(ts, m.pisum0, m.stats, PRIORS, pi_set)
    twins = m.rep != np.arange(m.K)
    for name, got, want in (('pi', pi_c, pi_e), ('theta', th_c, th_e)):
        bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
        assert len(bad) == 0, (label, name, 'differs from the closed form in columns', bad[:5], got[bad[:5]], want[bad[:5]], 'twins:', twins[bad[:5]])
    merged = twins & took
    assert np.array_equal(th_c[merged], th_c[m.rep[merged]]), (label, 'a twin within 1e-12 of its representative has another theta')
    apart = twins & ~took
    lim = E.diff_bound(m.K, diff_e)
    dfrac = float(abs(LD(diff) - diff_e) / lim) if lim > 0 else (0.0 if diff == float(diff_e) else np.inf)
    assert dfrac <= 1.0, (label, 'diff_est', diff, float(diff_e), dfrac)
    return dfrac, pi_c, th_c, int(merged.sum()), int(apart.sum())


def _forms(m):
    """the lnl forms a layout has: the fused_dbg bits select among the forms of the fused kernel's lnl pass; elsewhere one form"""
    i = m.info
    return FORMS if (i['fused'] == 1 and i['split'] == 0 and i['nb'] > 0 and i['reproducible'] == 0) else (0,)


def _leg(m, mkey, pnames, label, forms=True, limit_of=None):
    """checks 1 - 4 for every parameter set; returns the largest fractions (column sums, lnl, diff_est).  forms: True every form the
    layout has, False the unforced pass alone, or the tuple of fused_dbg values to run"""
    top = [0.0, 0.0, 0.0]
    for pname in pnames:
        ref = _ref(mkey, m.raw, pname)
        lab = '%s/%s/%s' % (label, mkey, pname)
        m.eng.set_params(ref.pi, ref.theta)
        m.eng.set_params(ref.pi, ref.theta)                         # previous = current
        lf = []
        for form in (forms if isinstance(forms, tuple) else (_forms(m) if forms else (0,))):
            m.eng.set_option('fused_dbg', form)
            lf.append(_check_lnl(m, ref, lab + '/form %d' % form))
        m.eng.set_option('fused_dbg', 0)
        f1, red = _check_pass(m, ref, lab, limit_of)
        df, pi_c, th_c, merged, apart = _check_update(m, red, ref.pi, ref.theta, lab)
        ref2 = E.PassReference(m.raw, m.lut, pi_c, th_c, ref.pi, ref.theta)
        assert ref2.fair == [], (lab, 'after the update', ref2.fair)
        f4, _ = _check_pass(m, ref2, lab + '/after update', limit_of)
        l4 = _check_lnl(m, ref2, lab + '/after update')
        _say('%s: column sums %.3f, after the update %.3f of the bound; lnl %s, after the update %.3g of its limit; diff_est %.3f of '
             'its bound; %d twins merged, %d apart; %d dead rows', lab, f1, f4, ' '.join('%.3g' % x for x in lf), l4, df, merged, apart,
             int((ref.state.amb & ~ref.state.live).sum()))
        top = [max(top[0], f1, f4), max(top[1], l4, *lf), max(top[2], df)]
    return top


def _assert_options_taken(info, options):
    for key, v in options:
        if key == 'parts':
            assert info['P'] == v, (options, info)
        if key == 'value_format':
            assert info['value_bytes'] == (2 if v == 2 else 8) and info['fused'] == 1, (options, info)
            if info['split'] == 0:
                assert info['index_bytes'] == (4 if v == 2 else 3), (options, info)
        if key == 'block_rows':
            assert info['R'] == v, (options, info)
        if key == 'split' and v == 1:
            assert info['split'] == 1 and info['fused'] == 1 and info['index_bytes'] == 4, (options, info)
        if key == 'em_kernel' and v == 1:
            assert info['fused'] == 0, (options, info)
        if key == 'hot_split':
            assert (info['hot_cols'] > 0) == (v == 1), (options, info)
        if key == 'reproducible':
            assert info['reproducible'] in (1, 2) and info['exact_single'] == (1 if v == 1 else 0), (options, info)
        if key == 'use_likelihood':
            assert info['lnl_fused'] == 1, (options, info)


# ---- the row-shape matrix on every rung -------------------------------------------------------------------------------------------
def _fmt_parts(parts, fmts=(1, 2)):
    return [(('parts', p), ('value_format', f)) for p in parts for f in fmts]


TEAM_LEGS = _fmt_parts((1, 2, 3, 4, 5, 7, 8))
SPLIT_LEGS = [(('split', 1),) + o for o in _fmt_parts((5, 8))]
OTHER_LEGS = [(('em_kernel', 1),), (('parts', 2), ('drop_csr_indices', 1)), (('parts', 2), ('use_likelihood', 1)), (('parts', 2), ('reproducible', 1)), (('parts', 2), ('reproducible', 2)),
              (('hot_split', 1),), (('hot_split', 0),)]


def _name(options):
    return '-'.join('%s%d' % (k, v) for k, v in options) or 'default'


def _geometry_ok(info, options):
    o = dict(options)
    if info['fused'] != 1 or info['split'] == 1 or 'parts' not in o:
        return True
    if o['parts'] == 1:
        return True
    return info['geometry'] == 0 if o['parts'] <= 4 else info['geometry'] in (1, 2)


@pytest.mark.parametrize('options', TEAM_LEGS + SPLIT_LEGS + OTHER_LEGS, ids=_name)
def test_row_shapes_on_every_rung(gpu_device, options):
    """The row-shape matrix (rows of 2 ... 1000 entries and one of K - 2, twins, a hot pair, a column of single-entry rows only, an
    empty column, empty rows) x every parameter set, checks 1 - 4, on the forced layout.  Where the long rows went is pinned from
    layout_info: a later layout change cannot silently move them."""
    hot = dict(options).get('hot_split') is not None
    # (one column part: the row of K - 2 entries must fit one register tile, see _em_pass_reference.matrix)
    mkey = 'zipf' if hot else ('row_shape_p1' if dict(options).get('parts') == 1 else 'row_shape')
    raw = E.matrix(mkey)
    m = Model(gpu_device, raw, options)
    info = m.info
    _assert_options_taken(info, options)
    assert _geometry_ok(info, options), (options, info)
    if dict(options).get('drop_csr_indices') == 1:
        assert m.eng.device_memory()['resident']['csr_indices'] == 0, 'the column ids are resident before the passes'
    limit_of = None
    if 'reproducible' in dict(options):
        limit_of = E.repro_limit
    top = _leg(m, mkey, SETS, _name(options), limit_of=limit_of)
    info = m.eng.layout_info()
    if dict(options).get('drop_csr_indices') == 1:
        assert m.eng.device_memory()['resident']['csr_indices'] == 0, 'the passes left the column ids resident'
    if 'reproducible' in dict(options):
        assert info['reproducible'] in (1, 2), ('a pass gave up moving a grid or a long row made a sum timing-dependent', info)
    _say('%s %s: P %d Kp %d R %d nb %d geometry %d fused %d split %d hot_cols %d slow_path %d single_part_rows %d max_subblock %d | largest: '
         'column sums %.3f lnl %.3g diff %.3f', _name(options), mkey, info['P'], info['Kp'], info['R'], info['nb'], info['geometry'], info['fused'],
         info['split'], info['hot_cols'], info['slow_path'], info['single_part_rows'], info['max_subblock'], *top)
    assert info['fallbacks'] == 0, info
    if info['fused'] == 1 and not hot:
        # where the long rows went: through the fused kernel's register tile (no fall-back layout), the row of K - 2 entries cut over
        # the P column parts — its largest share sits in ONE sub-block, and no sub-block exceeds a tile (3584 entries; 3328 with three
        # exchange waves); rows that live in a single part exist (the short ones) and are counted
        cap = 3584 if info['geometry'] == 0 else 3328
        assert -(-(m.K - 2) // info['P']) <= info['max_subblock'] <= cap, info
        assert 0 < info['single_part_rows'] <= info['N_amb'], info
    if dict(options).get('em_kernel') == 1:
        assert info['max_subblock'] == 0 and info['single_part_rows'] == 0 and info['R'] == 2048, info   # the two-pass layout: blocks of R rows, no tiles


# ---- steady state: the rings wrap -------------------------------------------------------------------------------------------------
def _ring_rows(cu_count, P, block_rows=64):
    """rows of the ring matrix so that every team walks at least 2 FZ_XS + 1 blocks (P > 1: the exchange ring wraps twice, a tag value
    returns) or 2 FZ_NS + 1 (P = 1: the register ring wraps twice): teams <= CUs // P, blocks are dealt round-robin, 5 % of the rows
    are single-entry rows and stay outside the blocks"""
    need = 2 * FZ_XS + 1 if P > 1 else 2 * FZ_NS + 1
    teams = max(1, cu_count // P)
    return need, teams, int(np.ceil((need + 1) * teams * block_rows / 0.93))


@pytest.mark.parametrize('options', TEAM_LEGS + SPLIT_LEGS + [(('parts', 4), ('reproducible', 1)), (('parts', 4), ('reproducible', 2))], ids=_name)
def test_rings_wrap_twice(gpu_device, cu_count, options):
    """Many blocks of short rows with the smallest block the layout takes (block_rows = 64): every team of the launch walks its
    exchange ring (8 slots) or its register ring (6 sets) round more than twice — asserted from nb and the team count — with dead
    rows and dying columns in the blocks.  Checks 1 - 4."""
    o = dict(options)
    need, teams, rows = _ring_rows(cu_count, o['parts'])
    raw = E.matrix('ring', rows)
    m = Model(gpu_device, raw, options + (('block_rows', 64),))
    info = m.info
    _assert_options_taken(info, options + (('block_rows', 64),))
    assert info['nb'] // teams >= need, ('a team walks fewer than %d blocks' % need, info, teams)
    limit_of = None
    if 'reproducible' in o:
        limit_of = E.repro_limit
    top = _leg(m, ('ring', rows), ('dead_rows', 'decades'), _name(options), forms=False, limit_of=limit_of)
    info = m.eng.layout_info()
    _say('%s ring: %d rows, %d blocks of %d rows over at most %d teams = %d blocks per team (>= %d) | largest: column sums %.3f lnl %.3g diff %.3f',
         _name(options), rows, info['nb'], info['R'], teams, info['nb'] // teams, need, *top)
    assert info['fallbacks'] == 0, info


@pytest.mark.parametrize('block_rows', [1152, 64])
def test_short_rows(gpu_device, block_rows):
    """rows of 2 - 6 entries: geometry 3 of the fused kernel, with the largest and the smallest block"""
    raw = E.matrix('short')
    m = Model(gpu_device, raw, (('block_rows', block_rows),))
    info = m.info
    assert info['fused'] == 1 and info['geometry'] == 3 and info['R'] == block_rows, info
    top = _leg(m, 'short', ('decades', 'dead_rows', 'subnormal'), 'short-%d' % block_rows)
    _say('short rows, block_rows %d: P %d nb %d | largest: column sums %.3f lnl %.3g diff %.3f', block_rows, info['P'], info['nb'], *top)


# ---- the upper rungs of the K ladder ----------------------------------------------------------------------------------------------
def test_natural_split_layout(gpu_device):
    raw = E.matrix('wide_70k')
    m = Model(gpu_device, raw)
    assert m.info['split'] == 1 and m.info['fused'] == 1, m.info
    top = _leg(m, 'wide_70k', ('decades', 'dead_rows'), 'split-natural')
    _say('K = 70 000: split layout, P %d Kp %d | largest: column sums %.3f lnl %.3g diff %.3f', m.info['P'], m.info['Kp'], *top)


def test_csr_row_passes(gpu_device):
    raw = E.matrix('wide_500k')
    m = Model(gpu_device, raw)
    assert m.info['row_pass_em'] == 1 and m.info['fused'] == 0, m.info
    top = _leg(m, 'wide_500k', ('decades', 'dead_rows'), 'row-passes')
    _say('K = 500 000: CSR row passes | largest: column sums %.3f lnl %.3g diff %.3f', *top)


def test_fallback_to_the_two_pass_kernels_keeps_the_parameters(gpu_device):
    """tsem_fallback_twopass on a fused handle after set_params: the layout is rebuilt, the parameters and the tables survive"""
    from telescope_amd._lib import Z_CUR, Z_PREV
    raw = E.matrix('row_shape')
    m = Model(gpu_device, raw, (('parts', 2),))
    assert m.info['fused'] == 1, m.info
    ref = _ref('row_shape', raw, 'dying')
    prev = _ref('row_shape', raw, 'decades')
    m.eng.set_params(prev.pi, prev.theta)
    m.eng.set_params(ref.pi, ref.theta)
    m.eng.fallback_twopass()
    m.info = m.eng.layout_info()
    assert m.info['fused'] == 0 and m.info['fallbacks'] == 1, m.info
    for which, want in ((Z_CUR, ref), (Z_PREV, prev)):
        pi, theta = m.eng.get_params(which)
        assert np.array_equal(pi.view(np.uint64), want.pi.view(np.uint64)) and np.array_equal(theta.view(np.uint64), want.theta.view(np.uint64))
    both = E.PassReference(raw, m.lut, ref.pi, ref.theta, prev.pi, prev.theta)
    assert both.fair == []
    lf = _check_lnl(m, both, 'fallback')                            # ctab_prev and ctab of the rebuilt layout
    f1, red = _check_pass(m, both, 'fallback')
    df = _check_update(m, red, ref.pi, ref.theta, 'fallback')[0]
    _say('fallback_twopass: column sums %.3f of the bound, lnl(prev, cur) %.3g of its limit, diff_est %.3f', f1, lf, df)


# ---- the forms of the lnl pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('options', [(('parts', 1), ('value_format', 2)), (('parts', 4), ('value_format', 2)), (('parts', 1), ('value_format', 1)),
                                     (('parts', 8), ('value_format', 1))], ids=_name)
def test_lnl_forms_straddle_their_limits(gpu_device, options):
    """Q pi theta above 2^27, below e^-40 and between the two in ONE pass, at two densities of the middle range: below the device's
    selection limit (0.1 % of the stored entries: the log-table form runs) and above it (the per-entry logarithm runs) — read from
    layout_info after the unforced pass.  Every form, forced and unforced, within the limit of the exact lnl."""
    raw = E.matrix('ring_hi')
    m = Model(gpu_device, raw, options)
    _assert_options_taken(m.info, options)
    for pname in ('lnl_straddle_sparse', 'lnl_straddle_dense'):
        ref = _ref('ring_hi', raw, pname)
        above, mid, below = E.straddle_counts(raw, m.lut, ref.pi, ref.theta)
        assert above > 0 and mid > 0 and below > 0, (pname, above, mid, below)
        m.eng.set_params(ref.pi, ref.theta)
        m.eng.set_params(ref.pi, ref.theta)
        lf, vals = [], []
        for form in FORMS:
            m.eng.set_option('fused_dbg', form)
            lf.append(_check_lnl(m, ref, '%s/%s/form %d' % (_name(options), pname, form)))
            vals.append(float(m.eng.read_reduce(m.K, 1)[0]))
            if form == 0:
                info = m.eng.layout_info()
        m.eng.set_option('fused_dbg', 0)
        _say('%s %s: the four forms give %d distinct values, %.1f ulp apart at most', _name(options), pname, len(set(vals)),
             (max(vals) - min(vals)) / np.spacing(abs(vals[0])))
        armed = info['lnl_tables'] > 0 or info['lnl_linear'] == 1
        _say('%s %s: %d / %d / %d entries above / between / below; device counted %d for the middle range, limit %d; lnl %s of its limit '
             '(unforced, per-entry log, table look-up, log form)', _name(options), pname, above, mid, below, info['lnl_mid_entries'], info['lnl_mid_limit'],
             ' '.join('%.3g' % x for x in lf))
        assert armed and info['lnl_mid_entries'] >= 0, ('the log-table form is not armed on this layout', info)
        if pname.endswith('sparse'):
            assert info['lnl_mid_entries'] <= info['lnl_mid_limit'], info    # the log-table form ran
        else:
            assert info['lnl_mid_entries'] > info['lnl_mid_limit'], info     # the per-entry logarithm ran
        f1, _ = _check_pass(m, ref, '%s/%s' % (_name(options), pname))
        _say('%s %s: column sums %.3f of the bound', _name(options), pname, f1)


# ---- the carried lnl (MODE 4) -----------------------------------------------------------------------------------------------------
def test_carried_lnl_over_chunks(gpu_device):
    """em_chunk over 3 iterations in chunks of 1 + 2 on a layout built for the carried lnl: the lnl of a chunk's last iteration is NaN
    when the chunk returns and arrives as the next chunk's carry (the last chunk flushes its own); each lnl_t is held against
    exact_lnl of the device's own parameters of that iteration, fetched between the chunks."""
    from telescope_amd._lib import Z_CUR, Z_PREV
    raw = E.matrix('ring', 40000)
    m = Model(gpu_device, raw, (('use_likelihood', 1), ('parts', 4), ('block_rows', 64)))
    assert m.info['lnl_fused'] == 1 and m.info['fused'] == 1 and m.info['P'] == 4, m.info
    start = _ref(('ring', 40000), raw, 'decades')
    m.eng.set_params(start.pi, start.theta)
    d1, l1, stopped = m.eng.em_chunk(1, 0.0, use_likelihood=True, first=True)
    assert len(d1) == 1 and not stopped and np.isnan(l1[0]) and np.isnan(m.eng.lnl_carry)      # nothing owed at entry; the value is owed now
    p0, p1 = m.eng.get_params(Z_PREV), m.eng.get_params(Z_CUR)
    assert np.array_equal(p0[0], start.pi) and np.array_equal(p0[1], start.theta)
    d2, l2, stopped = m.eng.em_chunk(2, 0.0, use_likelihood=True, last=True)
    carry = m.eng.lnl_carry
    assert len(d2) == 2 and not stopped and np.isfinite(carry) and np.all(np.isfinite(l2))
    p2, p3 = m.eng.get_params(Z_PREV), m.eng.get_params(Z_CUR)
    assert E.fair_stops(np.abs(np.diff([carry, l2[0], l2[1]])), 0.0) == []          # (epsilon = 0: no stop test can fire)
    fr = []
    for t, (lnl, prev, cur) in enumerate(((carry, p0, p1), (l2[0], p1, p2), (l2[1], p2, p3)), 1):
        ref = E.PassReference(raw, m.lut, cur[0], cur[1], prev[0], prev[1])
        assert ref.fair == [], (t, ref.fair)
        fr.append(float(abs(LD(lnl) - ref.lnl) / ref.lnl_limit_P(4)))
        assert fr[-1] <= 1.0, ('lnl of iteration', t, lnl, float(ref.lnl), fr[-1])
    _say('carried lnl, chunks 1 + 2: lnl_1 (carry) %.3g, lnl_2 %.3g, lnl_3 (flushed) %.3g of their limits', *fr)
    assert m.eng.layout_info()['fallbacks'] == 0


# ---- sharding ---------------------------------------------------------------------------------------------------------------------
def test_shards_cut_inside_a_run_of_long_rows(gpu_device):
    """The row-shape matrix with its rows sorted by length, cut between two of the 1000-entry rows: each shard's red is within bound
    of the exact sums of ITS rows (not just additive)."""
    raw = E.matrix('row_shape')
    lens = np.diff(raw.indptr)
    order = np.argsort(lens, kind='stable')
    srt = raw[order]
    srt.sort_indices()
    cut = int(np.flatnonzero(np.diff(srt.indptr) == 1000)[1])
    assert np.diff(srt.indptr)[cut - 1] == 1000 and np.diff(srt.indptr)[cut] == 1000
    pi, theta = E.parameter_set('dying', raw)
    for name, shard in (('head', srt[:cut]), ('tail', srt[cut:])):
        shard = shard.tocsr()
        shard.sort_indices()
        m = Model(gpu_device, shard, lut=E.lut(raw))
        ref = E.PassReference(shard, m.lut, pi, theta)
        assert ref.fair == []
        m.eng.set_params(pi, theta)
        m.eng.set_params(pi, theta)
        f1, _ = _check_pass(m, ref, 'shard ' + name)
        lf = _check_lnl(m, ref, 'shard ' + name)
        _say('shard %s: %d rows, longest %d: column sums %.3f of the bound, lnl %.3g of its limit; fused %d P %d', name, shard.shape[0],
             int(np.diff(shard.indptr).max()), f1, lf, m.info['fused'], m.info['P'])


# ---- option "reproducible": two engines, the same bits ----------------------------------------------------------------------------
@pytest.mark.parametrize('form', [1, 2])
def test_reproducible_engines_agree_bit_for_bit(gpu_device, form):
    """Two engines over one matrix (rows of at most 12 entries: every row's partial sum is one run), the same parameters: the column
    sums of a pass, and of the pass after the update, are the same bits — and within the documented bound of the exact sums."""
    raw = E.matrix('ring', 40000)
    options = (('parts', 4), ('reproducible', form), ('block_rows', 64))
    ms = [Model(gpu_device, raw, options) for _ in range(2)]
    for m in ms:
        _assert_options_taken(m.info, options)
    limit_of = E.repro_limit
    for pname in ('decades', 'dying'):
        ref = _ref(('ring', 40000), raw, pname)
        reds, after = [], []
        for m in ms:
            m.eng.set_params(ref.pi, ref.theta)
            f1, red = _check_pass(m, ref, 'reproducible %d/%s' % (form, pname), limit_of)
            reds.append(red)
            m.eng.em_update()
            m.eng.em_pass()
            after.append(m.eng.read_reduce(0, m.K + 2))
            info = m.eng.layout_info()
            assert info['reproducible'] == 1, ('the sums are not guaranteed exact', info)
        assert np.array_equal(reds[0].view(np.uint64), reds[1].view(np.uint64)), (form, pname, 'the pass')
        assert np.array_equal(after[0].view(np.uint64), after[1].view(np.uint64)), (form, pname, 'the pass after the update')
        _say('reproducible %d %s: two engines bit-equal; column sums %.3f of the documented bound; %d repeated passes', form, pname, f1, info['bin_repeats'])
