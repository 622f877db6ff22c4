"""CPU (`-m "not gpu"`): ties tests/_em_pass_reference.py down before tests/test_gpu_em_pass_exact.py holds the EM pass, the lnl pass
and the update kernel against it.

* on every matrix x parameter set of the GPU file, at reduced size: the input is fair, and the oracle's own fp64 results
  (estep -> z.multiply(weights).multiply(Y).sum(0), calculate_lnl, mstep of oracle/telescope_oracle.py) lie within the bounds the
  kernels are held to, with P = 0 and no tag term — the bounds are satisfiable by a correct fp64 implementation;
* the same against oracle/em_fused.c for one iteration;
* degenerate rows: an all-dead row contributes 0 and no NaN, a subnormal product takes fp64's value;
* fair() rejects constructed unfair inputs; the twin representatives and the closed forms of the update.

Each test prints the figures it asserts on (`pytest -s`)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _em_pass_reference as E
import _rowpass_reference as R

LD = E.LD


def _case(mname, pname):
    raw = E.matrix(mname, E.REDUCED.get(mname))
    pi, theta = E.parameter_set(pname, raw)
    return raw, E.lut(raw), pi, theta


@pytest.mark.parametrize('pname', E.PARAMETER_SETS)
@pytest.mark.parametrize('mname', E.MATRICES)
def test_the_oracle_is_within_the_bounds_and_the_input_is_fair(mname, pname):
    raw, lut, pi, theta = _case(mname, pname)
    k = raw.shape[1]
    ref = E.PassReference(raw, lut, pi, theta)
    assert ref.fair == [], (mname, pname, ref.fair)
    if True:
        assert abs(pi.sum() - 1) < 1e-9 and abs(theta.sum() - 1) < 1e-9
    sums, lnl, om = E.oracle_pass(raw, lut, pi, theta)
    limit = E.colsum_bound(ref.cnt, ref.lenmax, E.ORACLE) * ref.sums + ref.gradual + ref.cnt * LD(E.ABS_SLACK) + E.oracle_slack(ref.state, k)
    frac, j = E.colsum_fraction(sums, ref.sums, ref.cnt, ref.lenmax, ref.gradual, limit=limit)
    lfrac = float(abs(LD(lnl) - ref.lnl) / ref.lnl_limit)
    dead = int((ref.state.amb & ~ref.state.live).sum())
    print('EMREF %s/%s: oracle column sums %.3f of the bound (column %d, %d entries), lnl %.3f of its bound, %d dead rows, %d columns at 0'
          % (mname, pname, frac, j, ref.cnt[j], lfrac, dead, int((ref.sums == 0).sum())))
    assert not np.any(np.isnan(sums)) and np.isfinite(lnl)
    assert frac <= 1.0 and lfrac <= 1.0
    assert np.all(sums[(ref.sums == 0) & (limit == 0)] == 0)
    if pname == 'dead_rows':
        assert dead >= 2
    if pname == 'subnormal':
        assert ref.state.gradual.any() and (ref.gradual > 0).any()
    if pname.startswith('lnl_straddle') and mname == 'ring_hi':
        above, mid, below = E.straddle_counts(raw, lut, pi, theta)
        assert above > 0 and mid > 0 and below > 0
        share = mid / raw.nnz
        assert share < 1e-3 if pname.endswith('sparse') else share > 1e-3, share
    # mstep: the oracle's closed forms are exact_update's, bit for bit, on the oracle's own sums
    om.total_wt, om.ambig_wt = om.weights.sum(), om.weights.multiply(om.Y).sum()
    wmax = om.weights.max()
    om.pi_prior_wt, om.theta_prior_wt = 0 * wmax, 200000 * wmax
    om.pisum0 = om.Q.multiply(1 - om.Y).sum(0)
    with np.errstate(over='ignore', under='ignore', divide='ignore'):
        pi_o, theta_o = om.mstep(om.estep(pi, theta))
    pi_e, theta_e, diff = E.exact_update(sums, np.asarray(om.pisum0).ravel(), (om.total_wt, om.ambig_wt, wmax), (0, 200000), pi)
    assert np.array_equal(pi_o, pi_e) and np.array_equal(theta_o, theta_e)
    assert abs(LD(np.abs(pi_o - pi).sum()) - diff) <= E.diff_bound(k, diff)


def test_previous_parameters_in_the_lnl():
    """z of one parameter set against the logarithms of another: the oracle within the bound; swapping the two is far outside it"""
    raw, lut, pi, theta = _case('row_shape', 'dying')
    pp, tp = E.parameter_set('decades', raw)
    ref = E.PassReference(raw, lut, pi, theta, pp, tp)
    assert ref.fair == []
    _, lnl, _ = E.oracle_pass(raw, lut, pi, theta, pp, tp)
    frac = float(abs(LD(lnl) - ref.lnl) / ref.lnl_limit)
    _, stale, _ = E.oracle_pass(raw, lut, pi, theta)
    print('EMREF lnl(prev, cur): %.3f of its bound; with z of the current parameters instead %.3g bounds away' % (frac, float(abs(LD(stale) - ref.lnl) / ref.lnl_limit)))
    assert frac <= 1.0 and abs(LD(stale) - ref.lnl) > 1e3 * ref.lnl_limit


@pytest.mark.parametrize('mname', ['row_shape', 'zipf', 'ring_hi'])
def test_the_c_oracle_is_within_the_bounds_for_one_iteration(mname):
    """oracle/em_fused.c from pi = theta = 1 / K, one iteration: theta_hat carries the column sum's error — |theta_c - theta| <=
    bound_j sum_j / theta_den + 2 x 2^-53 theta (the addition and the division) — and the final lnl is calculate_lnl(z(1 / K), the
    C oracle's own new parameters)."""
    from oracle import em_fused as oc
    raw = E.matrix(mname, E.REDUCED.get(mname))
    lut, k = E.lut(raw), raw.shape[1]
    assert np.array_equal(lut, oc.score_lut(int(raw.data.max())))     # (the C oracle builds its table from the largest stored score)
    u = np.full(k, 1.0 / k)
    r = oc.em_fused_arrays(raw.indptr, raw.indices, raw.data, k, 0, 200000, 0.0, 1)
    ref = E.PassReference(raw, lut, u, u, want_lnl=False)
    assert ref.fair == []
    st = ref.state
    w_amb, w_max = LD(st.w[st.amb].astype(LD).sum()), LD(st.w.max())
    tpw = LD(200000) * w_max
    tden = w_amb + tpw * k
    theta = (ref.sums + tpw) / tden
    lim = (E.colsum_bound(ref.cnt, ref.lenmax, E.ORACLE) * ref.sums) / tden + 2 * LD(E.U) * theta + LD(3 * E.U) * theta   # (+ W_amb, tden: 3 more roundings)
    frac = float((np.abs(r['theta'].astype(LD) - theta) / lim).max())
    after = E.PassReference(raw, lut, r['pi'], r['theta'], u, u)
    lfrac = float(abs(LD(r['lnl']) - after.lnl) / after.lnl_limit)
    print('EMREF %s: em_fused.c theta_hat %.3f of its bound, lnl %.3f of its bound' % (mname, frac, lfrac))
    assert r['n_iter'] == 1 and frac <= 1.0 and lfrac <= 1.0


def test_degenerate_rows():
    """a row whose every column is dead contributes 0 and no NaN (recip0); a subnormal product takes fp64's value"""
    lut = E.lut()
    raw = sp.csr_matrix((np.array([212, 100, 50, 212, 7, 212, 30], dtype=np.uint16), np.array([0, 1, 2, 3, 0, 4, 1]), np.array([0, 3, 5, 7])), shape=(3, 5))
    pi = np.array([0.5, 0.25, 0.0, 0.0, 1e-160])
    theta = np.array([1.0, 0.5, 0.3, 0.0, 1e-160])
    pi[0] = 0.0                                                     # row 1 = columns (3, 0): both dead
    ref = E.PassReference(raw, lut, pi, theta)
    assert ref.fair == []
    assert not ref.state.live[1] and ref.state.live[0] and ref.state.live[2]
    assert not np.any(np.isnan(ref.sums.astype(np.float64))) and np.isfinite(float(ref.lnl))
    assert ref.sums[0] == 0 and ref.sums[3] == 0 and ref.sums[2] == 0 and ref.cnt[0] == 0
    c4 = pi[4] * theta[4]
    assert 0 < c4 < E.TINY
    n4 = float(ref.state.n[5])
    assert n4 == lut[212] * c4                                      # fp64's (pi theta), then an exact product in long double: no second rounding
    assert 0 < ref.sums[4] < 1e-200 and abs(float(ref.sums[1] + ref.sums[4]) / (2 * lut[212]) - 1) < 1e-15   # rows 0 and 2: z sums to 1, w = lut[212]
    sums, lnl, _ = E.oracle_pass(raw, lut, pi, theta)
    assert not np.any(np.isnan(sums)) and sums[0] == 0 and sums[3] == 0


def test_fair_rejects_unfair_inputs():
    lut = E.lut()
    raw = sp.csr_matrix((np.array([212, 200, 212, 100], dtype=np.uint16), np.array([0, 1, 2, 3]), np.array([0, 2, 4])), shape=(2, 4))
    ok = E.fair(raw.indptr, raw.indices, raw.data, lut, np.full(4, 0.25), np.full(4, 0.25))
    assert ok == []
    pi = np.array([1e-155, 1e-155, 0.5, 0.5])                       # row 0: every column at 1e-305: w / S = 1e305 >= 2^1000
    why = E.fair(raw.indptr, raw.indices, raw.data, lut, pi, np.array([1e-150, 1e-150, 1.0, 1.0]))
    assert len(why) == 1 and 'w / S' in why[0], why
    low = sp.csr_matrix((np.array([1, 1, 212, 100], dtype=np.uint16), raw.indices, raw.indptr), shape=(2, 4))
    why = E.fair(low.indptr, low.indices, low.data, lut, np.array([1e-160, 1e-160, 0.5, 0.5]), np.array([1e-150, 1e-150, 1.0, 1.0]))
    assert any('recip0' in x for x in why), why                     # a row sum of about 1e-310
    why = E.fair(raw.indptr, raw.indices, raw.data, lut, np.array([np.nan, 0.1, 0.5, 0.4]), np.full(4, 0.25))
    assert any('pi' in x for x in why)
    assert E.fair_stops([1e-3, 1.0000001e-7, 5e-8], 1e-7) == [1] and E.fair_stops([1e-3, 2e-7], 1e-7) == [] and E.fair_stops([0.0], 0.0) == []


def test_twin_representatives_and_the_twin_rule():
    cnt = np.array([5, 5, 0, 3, 5, 0, 3], dtype=np.uint64)
    hsh = np.array([9, 9, 0, 1, 8, 0, 1], dtype=np.uint64)
    assert E.twin_representatives(cnt, hsh).tolist() == [0, 0, 2, 3, 4, 5, 3]
    v, took = E.twin_rule(np.array([1.0, 1.0 + 1e-13, 0.0, 2.0, 7.0, 0.0, 2.1]), np.array([0, 0, 2, 3, 4, 5, 3]))
    assert v.tolist() == [1.0, 1.0, 0.0, 2.0, 7.0, 0.0, 2.1] and took.tolist() == [True, True, True, True, True, True, False]
    raw, special = E.row_shape_matrix()
    csc = raw.tocsc()
    for a, b in (special['hot'], special['twin']):
        assert np.array_equal(csc[:, a].indices, csc[:, b].indices) and np.array_equal(csc[:, a].data, csc[:, b].data)
