"""CPU: tests/_group_pass_reference.py — the exact single-step reference of the per-group EM fits — tied down before a GPU sees it.

 * against the oracle: step t of the reference, evaluated on the oracle's own state of step t - 1, reproduces OracleModel's
   estep / mstep / calculate_lnl on the group's rows (max_score of the whole matrix, as CellRef runs it) to the reference's own
   bounds, for t = 1 .. T on every case, and OracleModel.em stops where the reference's stop tests say;
 * against the emulation: the fp64 emulation of the device's arithmetic (`emulate`: _cell_em_reference.emulate_cell keeping every
   step; column sums in scipy's order = the one-lane order) stays within every bound on every case and step, and so does a second
   emulation that adds the columns in the spread tiers' piece-and-tree orders;
 * the bounds are not vacuous: the largest relative bound of any column sum and of any parameter is below 1e-12; 2^-30 of a column's
   sum added to it, and one z below 1e-12 of its row lost, both fail the checks;
 * the conditions on the inputs, for every case: every step of every group is fair, the stop margins hold, every extreme group
   meets a parameter that is exactly 0, a subnormal product and an entry that leaves z's pattern within T steps, every leg with a
   stop has a group that stops before T and one that does not (the spread case: one before, one at and one after the host's look).
No row, column, group, step or order is left out of any comparison.  `pytest -s` prints the `GROUPPASS-CPU` lines;
profiles/r31_group_pass_exact.txt keeps a run."""
import warnings

import numpy as np
import pytest

import _group_em_reference as G
import _group_pass_reference as P
import _rowpass_reference as R

MULTI = [(name, leg[0]) for name in ('classes', 'spread') for leg in P.LEGS]
DEGENERATE = [(key, priors) for key in P.DEGENERATE for priors in P.DEGENERATE_PRIORS]
_seen = {}                                        # (case, leg) -> the relative bounds met, for test_bounds_are_not_vacuous


def _say(fmt, *a):
    print('GROUPPASS-CPU ' + fmt % a, flush=True)


def _line(label, worst, **figures):
    _say('%s %s | %s', label, ' '.join('%s=%s' % kv for kv in sorted(figures.items())),
         ' '.join('%s %.3g' % (k, v[0]) for k, v in sorted(worst.items())))


def _walk(cs, priors, trs, label, worst, flags=None, rel=None):
    """every group and step of the trajectories `trs` against the reference evaluated on the trajectory's own previous state"""
    for g, tr in zip(cs.groups(), trs):
        pi, th = g.start()
        for t, s in enumerate(tr, 1):
            st = P.Step(g, priors, pi, th)
            assert st.fair == [], (label, g.c, t, 'the reference calls this step unfair', st.fair)
            P.check_step(st, s, worst, (label, 'group', g.c, 'step', t))
            if flags is not None:
                f = flags.setdefault(g.c, dict(zero=0, gradual=0, left=0))
                for k in f:
                    f[k] += int(st.flags[k])
            if rel is not None:
                a, b = st.relative_bounds()
                rel[0], rel[1] = max(rel[0], a), max(rel[1], b)
            pi, th = s['pi_dense'], s['theta_dense']


@pytest.mark.parametrize('name,leg', MULTI)
def test_emulation_stays_within_every_bound(name, leg):
    cs = P.case(name)
    _, pp, tp, use_lnl, stops = P.LEG[leg]
    eps = P.leg_eps(name, leg)
    flags, rel = {}, [0.0, 0.0]
    for order in (P.LANE, P.TIERS):
        worst = {}
        trs = P.trajectories(name, leg, order)
        assert all(len(tr) == cs.T for tr in trs)
        _walk(cs, (pp, tp), trs, (name, leg, order), worst, flags if order == P.LANE else None, rel)
        _line('emulation', worst, case=name, leg=leg, order=order, groups=cs.n_groups, steps=cs.T)
    _seen[(name, leg)] = rel
    # ---- the conditions on the inputs ----
    xs = [[s['x'] for s in tr] for tr in P.trajectories(name, leg)]
    assert P.stop_margin_failures(xs, eps) == [], (name, leg, eps)
    if stops:
        st = P._stop_steps(xs, eps)
        assert any(t is not None and t < cs.T for t in st) and any(t is None or t >= cs.T for t in st), (name, leg, st)
        if cs.spread:
            assert any(t is not None and t < G.SP_LOOK for t in st) and G.SP_LOOK in st and any(t is not None and t > G.SP_LOOK for t in st), st
        for g, tr, t in zip(cs.groups(), P.trajectories(name, leg), st):           # a stopped fit is the trajectory cut at its stop
            cut = P.emulate(g, (pp, tp), cs.T, eps, use_lnl)
            assert len(cut) == (t or cs.T) and all(np.array_equal(a['pi'], b['pi'], equal_nan=True) for a, b in zip(cut, tr))
        _say('stops case=%s leg=%s eps=%.6g steps=%s', name, leg, eps, ','.join(str(t) for t in st))
    else:
        assert eps == 0.0
        for c in cs.gadget_groups:                                              # the extreme groups of the extreme leg
            assert all(flags[c][k] > 0 for k in ('zero', 'gradual', 'left')), (name, c, flags[c])
        _say('extreme case=%s %s', name, ' '.join('group%d=zero:%d,subnormal:%d,left:%d' % (c, flags[c]['zero'], flags[c]['gradual'], flags[c]['left'])
                                                   for c in cs.gadget_groups))


@pytest.mark.parametrize('key,priors', DEGENERATE)
def test_emulation_of_the_degenerate_groups(key, priors):
    cs = P.degenerate_case(key, 0)
    for order in (P.LANE, P.TIERS):
        worst = {}
        trs = [P.emulate(g, priors, cs.T, 0.0, False, order) if len(g.rows) else [] for g in cs.groups()]
        _walk(cs, priors, trs, (key, priors, order), worst)
        _line('degenerate', worst, case=key, priors='%s/%s' % priors, order=order)
    if key == 'unique_only' and priors[1] == 0:
        s = P.emulate(cs.group(0), priors, 2)
        assert np.all(np.isnan(s[0]['theta'])) and np.all(np.isnan(s[1]['z'])) and np.isnan(s[0]['lnl'])
        assert len(cs.group(1).rows) == 0


def _oracle_steps(cs, g, priors, T, use_lnl):
    """OracleModel on the group's rows, stepped by hand: [(pi_prev, theta_prev, dict like emulate's)]"""
    from oracle.telescope_oracle import OracleModel
    om = OracleModel(g.sub, priors[0], priors[1], max_score=int(cs.raw.max()))
    assert np.array_equal(om.Q.data, g.q64), 'the score table is not the oracle\'s Q'
    K = g.K
    rest = lambda num, den: (np.float64(num) / np.float64(den))
    out = []
    pi, th = om.pi, om.theta
    with np.errstate(all='ignore'):
        for t in range(T):
            z = om.estep(pi, th)
            pi2, th2 = om.mstep(z)
            lnl = float(om.calculate_lnl(z, pi2, th2))
            za = R.align(z, g.sub, fill=np.nan)
            out.append((pi, th, dict(z=za, pi=pi2[g.cols], theta=th2[g.cols], lnl=lnl,
                                     rest_pi=rest(om.pi_prior_wt, om.total_wt + om.pi_prior_wt * K),
                                     rest_th=rest(om.theta_prior_wt, om.ambig_wt + om.theta_prior_wt * K),
                                     x=abs(lnl - (out[-1][2]['lnl'] if out else np.inf)) if use_lnl else float(np.abs(pi2 - pi).sum()))))
            pi, th = pi2, th2
    return out


@pytest.mark.parametrize('name,leg', MULTI)
def test_reference_reproduces_the_oracle(name, leg):
    from oracle.telescope_oracle import OracleModel
    cs = P.case(name)
    _, pp, tp, use_lnl, stops = P.LEG[leg]
    eps = P.leg_eps(name, leg)
    worst = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for g in cs.groups():
            steps = _oracle_steps(cs, g, (pp, tp), cs.T, use_lnl)
            for t, (pi, th, got) in enumerate(steps, 1):
                st = P.Step(g, (pp, tp), pi, th)
                P.check_step(st, got, worst, (name, leg, 'oracle', 'group', g.c, 'step', t))
            # OracleModel.em stops where the stop tests of its own steps say
            om = OracleModel(g.sub, pp, tp, max_score=int(cs.raw.max()))
            with np.errstate(all='ignore'):
                om.em(eps, cs.T, use_lnl)
            hit = [t for t, s in enumerate(steps, 1) if s[2]['x'] < eps]
            assert om.n_iter == (hit[0] if hit else cs.T) and bool(om.converged) == bool(hit and hit[0] <= cs.T), (name, leg, g.c, om.n_iter, hit)
            assert P._stop_steps([[s[2]['x'] for s in steps]], eps) == P._stop_steps([[s['x'] for s in P.trajectories(name, leg)[g.c]]], eps)
    _line('oracle', worst, case=name, leg=leg, groups=cs.n_groups, steps=cs.T)


@pytest.mark.parametrize('key,priors', DEGENERATE)
def test_reference_reproduces_the_oracle_on_the_degenerate_groups(key, priors):
    cs = P.degenerate_case(key, 0)
    worst = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for g in cs.groups():
            if len(g.rows) == 0:
                continue
            for pi, th, got in _oracle_steps(cs, g, priors, cs.T, False):
                P.check_step(P.Step(g, priors, pi, th), got, worst, (key, priors, 'oracle', 'group', g.c))
    _line('oracle_degenerate', worst, case=key, priors='%s/%s' % priors)


def test_bounds_are_not_vacuous():
    """the relative bounds met by the cases above; a column sum that is 2^-30 of itself too large and a lost z below 1e-12 of its
    row fail the checks"""
    for key in MULTI:
        if key not in _seen:                                                    # (run alone: walk the case here)
            test_emulation_stays_within_every_bound(*key)
    col = max(v[0] for v in _seen.values())
    par = max(v[1] for v in _seen.values())
    _say('bounds largest_relative_colsum=%.4g largest_relative_parameter=%.4g', col, par)
    assert 0 < col < 1e-12 and 0 < par < 1e-12, (col, par)      # (the longest columns hold unique rows' entries too: they add 0)
    cs = P.case('spread')
    priors = P.LEG['extreme'][1:3]
    # a. 2^-30 of the sum of the 4097-entry column (group 3) at step 3
    g = cs.group(3)
    j = int(g.cols[np.argmax(g.n_col[g.cols])])
    n_j = int(g.n_col[j])
    assert n_j == G.SP_WAVE + 1
    for order in (P.LANE, P.TIERS):
        trs = [P.emulate(g, priors, 3, order=order, tamper={'sum': (3, j, 2.0 ** -30)})]
        with pytest.raises(AssertionError, match='pi|theta'):
            _walk(_One(g), priors, trs, 'tampered sum', {})
    # b. one z below 1e-12 of its row, in the gadget's group: the step at which the trajectory first holds one
    g = cs.group(P.SPREAD_GADGET)
    clean = P.trajectories('spread', 'extreme')[P.SPREAD_GADGET]
    found = [(t, e) for t, s in enumerate(clean, 1) for e in np.flatnonzero((s['z'] > 0) & (s['z'] < 1e-12))[:1]]
    assert found, 'no z below 1e-12 on the trajectory'
    t, e = found[0]
    trs = [P.emulate(g, priors, t, tamper={'lose_z': (t, int(e))})]
    with pytest.raises(AssertionError):
        _walk(_One(g), priors, trs, 'lost z', {})
    _walk(_One(g), priors, [clean[:t]], 'untampered', {})
    _say('tamper sum_column=%d entries=%d lost_z=%.3g at step %d: both fail', j, n_j, clean[t - 1]['z'][e], t)


class _One(object):
    """a case of one group, for _walk"""
    def __init__(self, g):
        self.g = g

    def groups(self):
        return [self.g]


def test_cases_are_what_the_legs_need():
    cs = P.case('classes')
    assert cs.class_counts() == (4, 3, 2, 1, 0) and cs.gadget_groups == P.CLASS_GADGETS
    assert sorted(len(g.cols) for g in cs.groups())[:3] == [1, 1, 2] and min(len(g.rows) for g in cs.groups()) == 1
    for c in cs.gadget_groups:
        assert len(cs.group(c).twin_classes()) >= 1
    sp_ = P.case('spread')
    assert sp_.class_counts()[4] == sp_.n_groups and all(x > 0 for x in sp_.spread_tiers()) and (sp_.cor < 0).any()
    assert sp_.T >= G.SP_LOOK + 2
    for key in P.DEGENERATE:
        for spread in (0, 1):
            d = P.degenerate_case(key, spread)
            assert sum(d.class_counts()) == d.n_groups
