"""A plain reference of ONE iteration of the per-group EM fits (tsem_cell_em of telescope_amd/csrc/tsem_cellem.hip: the wave, 256-thread,
512-thread, global-workspace and spread classes), the rounding bounds it is held to, and the cases that
tests/test_group_pass_reference.py (CPU: this reference against the oracle and against an fp64 emulation of the device's arithmetic)
and tests/test_gpu_group_pass_exact.py (GPU: the HIP kernels against this reference) share.

The method.  The unit cannot be given a parameter state and does not need one: it is deterministic, a group's bits depend on the
group and its class alone, so the run with max_iter = t repeats the first t - 1 iterations of the run with max_iter = t - 1 bit for
bit.  Everything run t returns is therefore an exact function of what run t - 1 returned (pi = theta = 1 / K for t = 1):
    z_t                          the E-step of (pi, theta)_{t-1} on the group's rows
    (pi, theta, rest)_t          the M-step of that z with the group's own weights' totals and pisum0
    lnl_t                        calculate_lnl(z_t, (pi, theta)_t)
`Step` evaluates these in long double on the state of step t - 1 AS THE CALLER HOLDS IT (the device's own numbers in the GPU file):
no rounding error is carried from step to step, every bound is that of a single pass.

numpy and np.longdouble only; RowState, exact_colsums, oracle_slack, exact_lnl, fair, fair_stops come from
tests/_em_pass_reference.py, bound / U / TINY / ABS_SLACK from tests/_rowpass_reference.py.  Nothing here touches the engine.

Every bound is a first-order count of the roundings of the code path it is used for, written next to the count.  None of them was
tuned on a kernel's output.

The ladder gadget (GADGET): a few rows on columns of their own, appended to a group.  Under priors (0, 0) the columns that a
neighbour with more support dominates fall through the subnormal range to exactly 0 within about ten iterations: subnormal
products pi theta, numerators that underflow, entries that leave z's pattern, parameters that are exactly 0 — states no fit from
1 / K with the default priors visits.  A DEAD ambiguous row (every numerator 0) cannot arise on a trajectory — a row's z sums to 1,
so its weight keeps one of its columns alive — and no case asks for one.
"""
import functools

import numpy as np
import scipy.sparse as sp

import _cell_em_reference as C
import _em_pass_reference as E
import _group_em_reference as G
import _rowpass_reference as R

LD = R.LD
U = R.U
TINY = R.TINY
ABS_SLACK = R.ABS_SLACK
T_STEPS = 12
# (name, pi_prior, theta_prior, use_likelihood, the leg stops): the three parameter sets of every multi-step leg
LEGS = (('extreme', 0, 0, False, False), ('stops', 0, 200000, False, True), ('lnl', 1, 5, True, True))
LEG = {l[0]: l for l in LEGS}
DEGENERATE_PRIORS = G.DEGENERATE_PRIORS

# ---- the ladder gadget ------------------------------------------------------------------------------------------------------------
# (rows, ((column, score of a table of 212), ...)): columns 0 - 6 are the ladder (1 is dominated by 0, 4 by 1's leftovers, ...), 7 and 8
# are exact twins (the same rows, the same scores)
GADGET = ((30, ((0, 100),)), (20, ((0, 100), (1, 90))), (10, ((2, 50), (3, 45))), (5, ((1, 90), (4, 80))), (3, ((4, 80), (5, 70))),
          (3, ((5, 70), (6, 65))), (4, ((7, 60), (8, 60))))
GADGET_COLS = 9
GADGET_ENTRIES = sum(n * len(e) for n, e in GADGET)
GADGET_SCALE = 212


def gadget_rows(first_col, max_score):
    """[(columns, scores)] per row of the gadget on the columns first_col .. first_col + 8, the scores scaled to a table of
    `max_score` (Q = expm1(100 score / max_score) keeps its ratios up to the rounding of the scores)"""
    out = []
    for n, entries in GADGET:
        cols = [first_col + c for c, _ in entries]
        scores = [max(1, int(round(s * max_score / float(GADGET_SCALE)))) for _, s in entries]
        out += [(cols, scores)] * n
    return out


def _stack(raw, cor, k_new, extra, groups_of_extra):
    """`raw` widened to k_new columns with the rows `extra` = [(columns, scores)] appended; their groups appended to cor"""
    raw = sp.csr_matrix(raw)
    lens = [len(c) for c, _ in extra]
    indptr = np.concatenate([raw.indptr, raw.indptr[-1] + np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([raw.indices] + [np.asarray(c, np.int32) for c, _ in extra]).astype(np.int32)
    data = np.concatenate([raw.data] + [np.asarray(s, np.uint16) for _, s in extra]).astype(np.uint16)
    m = sp.csr_matrix((data, indices, indptr), shape=(raw.shape[0] + len(extra), k_new))
    m.sort_indices()
    return m, np.concatenate([np.asarray(cor, np.int32), np.asarray(groups_of_extra, np.int32)])


# ---- one group's fixed data -------------------------------------------------------------------------------------------------------
class Group(object):
    """What does not change from step to step for one group of a case: its rows, their entries, the weights' exact totals, pisum0."""

    def __init__(self, raw, cor, c, lut):
        self.c, self.K = c, raw.shape[1]
        self.rows = np.flatnonzero(np.asarray(cor) == c)
        self.sub = sub = sp.csr_matrix(raw[self.rows]) if len(self.rows) else sp.csr_matrix((0, self.K), dtype=np.uint16)
        self.indptr = sub.indptr.astype(np.int64)
        self.indices, self.data, self.lut = sub.indices, sub.data, np.asarray(lut, dtype=np.float64)
        self.lens = np.diff(self.indptr)
        self.rid = R.row_ids(self.indptr)
        full_ip = raw.indptr.astype(np.int64)
        self.ent = (np.concatenate([np.arange(full_ip[r], full_ip[r + 1]) for r in self.rows]).astype(np.int64)
                    if len(self.rows) else np.zeros(0, np.int64))            # the group's entries in the whole matrix's CSR order
        self.cols = np.unique(self.indices)
        self.touched = np.zeros(self.K, bool)
        self.touched[self.cols] = True
        self.q64 = self.lut[self.data]
        self.amb = self.lens > 1
        self.w = R._row_reduce(np.maximum, self.q64, self.indptr, 0.0) if len(self.lens) else np.zeros(0)
        wl = self.w.astype(LD)
        self.tw, self.aw = wl.sum(), wl[self.amb].sum()                      # exact up to rows 2^-64
        self.wm = float(self.w.max()) if len(self.w) else 0.0                # a maximum is exact
        self.rows_w = int((self.w > 0).sum())                                # rows whose weight is not 0: adding a 0 is exact
        self.rows_a = int(((self.w > 0) & self.amb).sum())
        uni = ~self.amb[self.rid]
        self.ps0 = E._sum_by(self.indices[uni], self.q64[uni].astype(LD), self.K)
        self.cnt_u = np.bincount(self.indices[uni & (self.q64 != 0)], minlength=self.K).astype(np.int64)
        self.n_col = np.bincount(self.indices, minlength=self.K).astype(np.int64)

    def twin_classes(self):
        """columns of the group with the same rows and the same scores (classes of two or more)"""
        csc = sp.csc_matrix(self.sub)
        seen = {}
        for j in self.cols:
            a, b = csc.indptr[j], csc.indptr[j + 1]
            seen.setdefault((csc.indices[a:b].tobytes(), csc.data[a:b].tobytes()), []).append(int(j))
        return [v for v in seen.values() if len(v) > 1]

    def dense(self, vals, rest):
        """a K-vector: `vals` on the touched columns, `rest` on the others"""
        out = np.full(self.K, rest, dtype=np.float64)
        out[self.cols] = vals
        return out

    def start(self):
        return np.full(self.K, 1.0 / self.K), np.full(self.K, 1.0 / self.K)


def _quot(num, den):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.asarray(num, dtype=LD) / LD(den)


def _ratio(a, b):
    """a / b with 0 / 0 = 0 (a share of a sum that is 0)"""
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    out = np.zeros(np.broadcast(a, b).shape, dtype=LD)
    ok = np.broadcast_to(b, out.shape) > 0
    out[ok] = (np.broadcast_to(a, out.shape)[ok] / np.broadcast_to(b, out.shape)[ok])
    return out


class Step(object):
    """Step t of one group from (pi, theta)_{t-1}, dense over the K columns (a column the group does not touch holds `rest`).

    z, inpat       exact z and its pattern on the group's entries (RowState: an entry whose fp64 numerator is exactly 0 is outside);
                   the bound per entry is _rowpass_reference.bound: (len + 3) 2^-53, one step of the subnormal grid absolute
    sums, sum_lim  the column sums over the ambiguous rows of w z and their ABSOLUTE limits.  ce_row_estep forms ((n rinv) w) y with
                   n = fl(Q fl(pi theta)): the oracle's sequence — five roundings per term (pi theta, Q c, 1 / S, n rinv, z w; the
                   factor y = 1 and the second term of tm_numer, + 0, are exact), len - 1 for the row sum, cnt - 1 for the column in
                   ANY order (the spread tiers change the order of a column's additions, not their number: a piece's sum, the tree
                   and the waves' sums are cnt - 1 additions of non-zero terms together, adding a 0 is exact):
                   colsum_bound(cnt, lenmax, ORACLE) = (lenmax + cnt + 3) 2^-53 relative, plus the `gradual` term (a numerator on
                   the subnormal grid), oracle_slack (z is formed before it meets w: a z below 2^-1022 sits on the subnormal
                   grid) and cnt 2^-1074 (a subnormal product z w)
    pi, theta, rest_pi, rest_th and their ABSOLUTE limits pi_lim, ...: the closed forms of tsem_model.h, see _mstep
    nan_state      the previous theta is NaN (a group without ambiguous rows at theta_prior = 0: 0 / 0): every numerator of the
                   group is NaN ((Q 0)(pi NaN) + Q pi), so z, pi, theta and lnl are NaN and the stop test is false"""

    def __init__(self, g, priors, pi_prev, theta_prev):
        self.g, self.priors = g, priors
        self.pi_prev = np.asarray(pi_prev, dtype=np.float64)
        self.theta_prev = np.asarray(theta_prev, dtype=np.float64)
        K = g.K
        bad = np.isnan(self.pi_prev[g.cols]) | np.isnan(self.theta_prev[g.cols])
        self.nan_state = bool(bad.any())
        if self.nan_state:
            assert bad.all() and not g.amb.any(), 'a NaN parameter in a group with ambiguous rows, or on some of its columns only'
        self.fair = []
        if self.nan_state or len(g.cols) == 0:
            self.state = None
            self.z = np.full(len(g.indices), np.nan if self.nan_state else 0.0, dtype=LD)
            self.inpat = np.ones(len(g.indices), bool)
            self.sums = np.full(K, np.nan if self.nan_state else 0.0, dtype=LD)
            self.sums[~g.touched] = 0
            self.sum_lim = np.zeros(K, dtype=LD)
            self.flags = dict(zero=False, gradual=False, left=False)
        else:
            p = np.where(g.touched, self.pi_prev, 0.0)                       # (the others are not read by the group's rows)
            t = np.where(g.touched, self.theta_prev, 0.0)
            a = (g.indptr, g.indices, g.data, g.lut)
            self.state = st = E.RowState(*a, p, t)
            self.fair = E.fair(*a, p, t, state=st)
            self.z, self.inpat = st.z, st.inpat
            self.sums, self.cnt, self.lenmax, self.gradual = E.exact_colsums(*a, p, t, state=st)
            self.abs_part = self.gradual + E.oracle_slack(st, K)
            self.sum_lim = E.colsum_bound(self.cnt, self.lenmax, E.ORACLE) * np.abs(self.sums) + self.abs_part + self.cnt.astype(LD) * LD(ABS_SLACK)
            self.flags = dict(zero=bool(np.any(p[g.cols] == 0) or np.any(t[g.cols] == 0)), gradual=bool(st.gradual.any()),
                              left=bool((~st.inpat).any()))
        self._mstep()

    def _mstep(self):
        """tm_prior, tm_theta, tm_pi in long double and the limits, first order, as counts of roundings:
          tpw = fl(theta_prior wm)                      1 (none where it is 0)
          den_th = fl(aw + fl(tpw K))                   aw: (ambiguous rows with a weight - 1) for ANY order of adding them (w y = 0 of
                                                        the other rows adds exactly); tpw K: tpw's rounding and the product's, 2, on
                                                        that part; the addition 1 (none where tpw = 0)
          theta = fl(fl(s + tpw) / den_th)              numerator: the column sum's limit, tpw's rounding, the addition 1 (none where
                                                        tpw = 0); the division 1
          pi = fl(fl(fl(ps0 + s) + ppw) / den_pi)       ps0: (unique entries of the column - 1) for any order; s: its limit; the first
                                                        addition 1 where both terms are not 0; ppw = fl(pi_prior wm) 1 and the second
                                                        addition 1 (none where ppw = 0); den_pi as den_th with tw (rows with a weight -
                                                        1); the division 1
          rest = fl(ppw / den_pi), fl(tpw / den_th)     (0 + 0) + ppw is exact: ppw's rounding, the denominator's, the division
        and one step of the subnormal grid (2^-1074) on a value that is not 0: a quotient below 2^-1022 is rounded onto that grid.
        A value whose exact value is 0 has the limit 0; 0 / 0 is NaN on both sides."""
        g, K = self.g, self.g.K
        pi_prior, theta_prior = self.priors
        u = LD(U)
        tpw, ppw = LD(theta_prior) * LD(g.wm), LD(pi_prior) * LD(g.wm)
        den_th, den_pi = g.aw + tpw * K, g.tw + ppw * K
        r_den_th = (_ratio(max(g.rows_a - 1, 0) * g.aw + 2 * tpw * K, den_th) + (1 if tpw != 0 else 0)) * u
        r_den_pi = (_ratio(max(g.rows_w - 1, 0) * g.tw + 2 * ppw * K, den_pi) + (1 if ppw != 0 else 0)) * u
        s, sl = self.sums, self.sum_lim
        num_th = s + tpw
        a_num_th = sl + (u * tpw + u * num_th if tpw != 0 else 0)
        self.theta = _quot(num_th, den_th)
        first = ((g.ps0 != 0) & (s != 0)).astype(LD)
        num_pi = (g.ps0 + s) + ppw
        a_num_pi = np.maximum(g.cnt_u - 1, 0).astype(LD) * u * g.ps0 + sl + first * u * (g.ps0 + s) + (u * ppw + u * num_pi if ppw != 0 else 0)
        self.pi = _quot(num_pi, den_pi)
        with np.errstate(invalid='ignore', divide='ignore'):
            self.theta_lim = a_num_th / den_th + np.abs(self.theta) * (r_den_th + u) + np.where(self.theta != 0, LD(ABS_SLACK), LD(0))
            self.pi_lim = a_num_pi / den_pi + np.abs(self.pi) * (r_den_pi + u) + np.where(self.pi != 0, LD(ABS_SLACK), LD(0))
        self.rest_pi, self.rest_th = _quot(ppw, den_pi), _quot(tpw, den_th)
        self.rest_pi_lim = np.abs(self.rest_pi) * ((1 if ppw != 0 else 0) * u + r_den_pi + u)
        self.rest_th_lim = np.abs(self.rest_th) * ((1 if tpw != 0 else 0) * u + r_den_th + u)

    def relative_bounds(self):
        """(largest relative limit of a column sum, of a parameter) over the touched columns whose exact value is not 0"""
        if self.nan_state or self.state is None:
            return 0.0, 0.0
        plain = self.g.touched & (self.abs_part == 0)                         # (the steps of the subnormal grid are no relative bound)

        def rel(lim, v):
            ok = plain & np.isfinite(v.astype(np.float64)) & (np.abs(v) >= LD(TINY))
            return float((lim[ok] / np.abs(v[ok])).max()) if ok.any() else 0.0
        return (float(E.colsum_bound(self.cnt, self.lenmax, E.ORACLE).max()),
                max(rel(self.pi_lim - LD(ABS_SLACK), self.pi), rel(self.theta_lim - LD(ABS_SLACK), self.theta)))

    def lnl(self, pi_cur, theta_cur):
        """(lnl_t, its absolute limit): exact_lnl with previous = (pi, theta)_{t-1}, current = the caller's (pi, theta)_t, P = 0"""
        g = self.g
        cur_nan = np.isnan(np.asarray(pi_cur)[g.cols]) | np.isnan(np.asarray(theta_cur)[g.cols])
        if self.nan_state or cur_nan.any():                                   # (theta_t = 0 / 0: every numerator of the current pair is NaN)
            assert self.nan_state or (cur_nan.all() and not g.amb.any())
            return LD(np.nan), LD(0)
        if len(g.cols) == 0:
            return LD(0), LD(0)
        p = np.where(g.touched, pi_cur, 0.0)
        t = np.where(g.touched, theta_cur, 0.0)
        lnl, lim, _ = E.exact_lnl(g.indptr, g.indices, g.data, g.lut, None, None, p, t, P=0, prev_state=self.state)
        return lnl, lim

    def diff(self, pi_cur):
        """sum over all K columns of |pi_t - pi_{t-1}| (model.py:781) of the caller's fp64 values, in long double: what the stop test
        of the parameter form compares with epsilon (its own rounding: K 2^-53 relative, far inside the margin of fair_stops)"""
        return np.abs(np.asarray(pi_cur, dtype=np.float64).astype(LD) - self.pi_prev.astype(LD)).sum()


def fraction(got, want, lim):
    """(largest |got - want| / lim, where): NaN must meet NaN; a limit of 0 asks for equality (inf otherwise)"""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    want, lim = np.atleast_1d(want).astype(LD), np.atleast_1d(lim).astype(LD)
    gn, wn = np.isnan(got), np.isnan(want.astype(np.float64))
    frac = np.zeros(len(got))
    frac[gn != wn] = np.inf
    ok = ~gn & ~wn
    with np.errstate(invalid='ignore'):
        err = np.abs(got.astype(LD) - want)
    pos = ok & (lim > 0)
    frac[pos] = (err[pos] / lim[pos]).astype(np.float64)
    frac[ok & ~(lim > 0) & (err != 0)] = np.inf
    j = int(np.argmax(frac)) if len(frac) else 0
    return (float(frac[j]) if len(frac) else 0.0), j


def check_step(step, got, worst=None, label=''):
    """Checks 2 - 4 of tests/test_gpu_group_pass_exact.py for one group and one step.  got: dict(z = the values on the group's entries
    (NaN = no entry), pi, theta = the values on the touched columns, rest_pi, rest_th, lnl).  Raises AssertionError; returns (and
    folds into `worst`) the largest error as a fraction of its limit per quantity."""
    worst = {} if worst is None else worst
    g = step.g

    def note(name, frac, j=0):
        if frac > worst.get(name, (-1.0,))[0]:
            worst[name] = (frac, label, j)
        assert frac <= 1.0, (label, name, 'index', j, 'fraction of its limit', frac)
    z = np.asarray(got['z'], dtype=np.float64)
    assert len(z) == len(g.indices), (label, 'z: entries')
    if step.nan_state:
        assert np.all(np.isnan(z)), (label, 'z of a group whose reference z is NaN has entries')
        note('z', 0.0)
    else:
        out = np.isnan(z)
        wrong = np.flatnonzero(out != ~step.inpat)
        assert len(wrong) == 0, (label, 'z: the pattern differs at entries', wrong[:5], z[wrong[:5]], step.inpat[wrong[:5]])
        fr = R.error_fraction(np.where(out, 0.0, z), step.z, step.inpat, g.indptr, per_entry=True)
        j = int(np.argmax(fr)) if len(fr) else 0
        note('z', float(fr[j]) if len(fr) else 0.0, j)
    for name, want, lim in (('pi', step.pi, step.pi_lim), ('theta', step.theta, step.theta_lim)):
        frac, j = fraction(got[name], want[g.cols], lim[g.cols])
        note(name, frac, int(g.cols[j]) if len(g.cols) else 0)
    for name, want, lim in (('rest_pi', step.rest_pi, step.rest_pi_lim), ('rest_th', step.rest_th, step.rest_th_lim)):
        note(name, fraction(got[name], want, lim)[0])                      # (the device reports the closed form even where Kc = K)
    pi_cur, th_cur = g.dense(got['pi'], got['rest_pi']), g.dense(got['theta'], got['rest_th'])
    lnl, lim = step.lnl(pi_cur, th_cur)
    note('lnl', fraction(got['lnl'], lnl, lim)[0])
    return worst


# ---- the fp64 emulation of the device's arithmetic ----------------------------------------------------------------------------------
LANE, TIERS = 'lane', 'tiers'


def _colsum(g, vals, order):
    """the column sums of `vals` (per entry of the group) in fp64: LANE — ascending row order from 0 (np.bincount adds in entry
    order: scipy's order, ce_col_sum); TIERS — the spread class's order by the column's entry count n: up to 32 one lane; up to 4096
    64 contiguous pieces of ceil(n / 64) and a tree over them; beyond 256 pieces of ceil(n / 256), a tree per 64 and the four sums in
    order"""
    K = g.K
    if order == LANE or len(vals) == 0:
        return np.bincount(g.indices, weights=vals, minlength=K)
    o = np.argsort(g.indices, kind='stable')
    col = g.indices[o]
    start = np.concatenate([[0], np.cumsum(g.n_col)])[:-1]
    rank = np.arange(len(col)) - start[col]
    n = g.n_col[col]
    m = np.where(n <= G.SP_LANE, np.maximum(n, 1), np.where(n <= G.SP_WAVE, -(-n // 64), -(-n // G.SP_T)))
    part = np.bincount(col.astype(np.int64) * 256 + rank // m, weights=vals[o], minlength=K * 256).reshape(K, 4, 64)
    for h in (32, 16, 8, 4, 2, 1):
        part = part[:, :, :h] + part[:, :, h:2 * h]
    part = part[:, :, 0]
    return ((part[:, 0] + part[:, 1]) + part[:, 2]) + part[:, 3]


def emulate(g, priors, T, eps=0.0, use_lnl=False, order=LANE, tamper=None):
    """The device unit's arithmetic for one group in fp64, step by step (tests/_cell_em_reference.emulate_cell, dense over the K
    columns and keeping every step): a list of dict(z, pi, theta (touched columns), rest_pi, rest_th, lnl, diff, x (the stop
    test's left side), converged, sums) for the steps the fit runs.  tamper: {'sum': (t, column, rel)} adds rel x the sum to one
    column sum of step t; {'lose_z': (t, entry)} loses one entry's z (and its contribution) at step t."""
    K = g.K
    tamper = tamper or {}
    pi_prior, theta_prior = priors
    y = g.amb[g.rid].astype(np.float64)
    q, w = g.q64, g.w
    tw, aw, wm = w.sum(), (w * g.amb).sum(), g.wm
    ppw, tpw = pi_prior * wm, theta_prior * wm
    den_th, den_pi = aw + tpw * K, tw + ppw * K
    ps0 = _colsum(g, q * (1.0 - y), order)
    pi, th = g.start()
    steps, lnl_prev = [], np.inf

    def numer(p, t):
        return (q * y) * (p * t)[g.indices] + (q * (1.0 - y)) * p[g.indices]
    with np.errstate(all='ignore'):
        for it in range(1, T + 1):
            n = numer(pi, th)
            rs = np.bincount(g.rid, weights=n, minlength=len(g.lens))
            r = 1.0 / rs
            r[np.isinf(r)] = 0.0
            z = n * r[g.rid]
            inp = n != 0.0
            contrib = np.where(inp, (z * w[g.rid]) * y, 0.0)
            z_out = np.where(inp, z, np.nan)
            if tamper.get('lose_z', (0,))[0] == it:
                e = tamper['lose_z'][1]
                contrib[e], z[e], z_out[e] = 0.0, 0.0, 0.0
            s = _colsum(g, contrib, order)
            if tamper.get('sum', (0,))[0] == it:
                _, j, rel = tamper['sum']
                s[j] += rel * s[j]
            th_new = (s + tpw) / den_th
            pi_new = ((ps0 + s) + ppw) / den_pi
            m = numer(pi_new, th_new)
            keep = inp & (m != 0.0)
            lnl = float((z[keep] * np.log1p(m[keep])).sum())
            diff = float(np.abs(pi_new - pi).sum())
            x = abs(lnl - lnl_prev) if use_lnl else diff
            conv = bool(x < eps)
            lnl_prev = lnl
            steps.append(dict(z=z_out, pi=pi_new[g.cols], theta=th_new[g.cols], rest_pi=ppw / den_pi, rest_th=tpw / den_th, lnl=lnl,
                              diff=diff, x=x, converged=conv, sums=s, pi_dense=pi_new, theta_dense=th_new))
            pi, th = pi_new, th_new
            if conv:
                break
    return steps


# ---- the cases --------------------------------------------------------------------------------------------------------------------
class Case(object):
    """raw (N x K, uint16), the group of every row (-1: none), the score table of the whole matrix, the spread option the leg sets,
    the groups that hold the gadget, the steps"""

    def __init__(self, name, raw, cor, n_groups, spread, gadget_groups=(), T=T_STEPS):
        from telescope_amd.likelihood import score_lut
        raw = sp.csr_matrix(raw)
        raw.sort_indices()
        self.name, self.raw, self.cor, self.n_groups = name, raw, np.asarray(cor, np.int32), int(n_groups)
        self.N, self.K = raw.shape
        self.lut = score_lut(int(raw.max())) if raw.nnz else score_lut(1)
        self.spread, self.gadget_groups, self.T = spread, tuple(gadget_groups), T
        self._groups = {}

    def group(self, c):
        if c not in self._groups:
            self._groups[c] = Group(self.raw, self.cor, c, self.lut)
        return self._groups[c]

    def groups(self):
        return [self.group(c) for c in range(self.n_groups)]

    def class_counts(self):
        """(wave, 256, 512, global, spread) by the documented rule, from the matrix alone"""
        out = [0, 0, 0, 0, 0]
        for g in self.groups():
            kc, ne = len(g.cols), len(g.indices)
            if self.spread > 0 and ne > self.spread:
                out[4] += 1
            else:
                out[0 if (kc <= 256 and ne <= 4096) else 1 if kc <= 1024 else 2 if kc <= 3840 else 3] += 1
        return tuple(out)

    def spread_tiers(self):
        """how many touched columns of spread groups fall into each tier (lane, wave, workgroup)"""
        out = [0, 0, 0]
        for g in self.groups():
            if self.spread > 0 and len(g.indices) > self.spread:
                n = g.n_col[g.cols]
                out[0] += int((n <= G.SP_LANE).sum()); out[1] += int(((n > G.SP_LANE) & (n <= G.SP_WAVE)).sum()); out[2] += int((n > G.SP_WAVE).sum())
        return tuple(out)


CLASS_GADGETS = (0, 1, 4, 6)                                  # one group of the wave, 256-thread, 512-thread and global-workspace class


@functools.lru_cache(maxsize=None)
def classes_case():
    """The cells of _cell_em_reference.B_CELLS — on either side of Kc 256 / 1024 / 3840 and of 4096 entries, Kc 1, Kc 2, one row —
    with the gadget appended to one cell of each class: that cell is laid over GADGET_COLS columns and GADGET_ENTRIES entries fewer,
    so that its Kc and its entry count are B_CELLS' again, on the stated side of the threshold."""
    cells = [(kc - GADGET_COLS, ne - GADGET_ENTRIES) if c in CLASS_GADGETS else (kc, ne) for c, (kc, ne) in enumerate(C.B_CELLS)]
    raw, cor, _ = C.boundary_matrix(C.B_SEED, C.B_K, cells)
    k = C.B_K
    for c in CLASS_GADGETS:
        rows = gadget_rows(k, int(raw.max()))
        raw, cor = _stack(raw, cor, k + GADGET_COLS, rows, [c] * len(rows))
        k += GADGET_COLS
    case = Case('classes', raw, cor, len(C.B_CELLS), 0, CLASS_GADGETS)
    for c, (kc, ne) in enumerate(C.B_CELLS):
        g = case.group(c)
        assert (len(g.cols), len(g.indices)) == (kc, ne), (c, len(g.cols), len(g.indices))
    assert case.class_counts() == (4, 3, 2, 1, 0)
    return case


SPREAD_GADGET = 0


@functools.lru_cache(maxsize=None)
def spread_case():
    """Every group spread (option cell_em_spread_entries = 1): the tier groups of _group_em_reference (columns of 32 | 33, 64 m |
    64 m + 1, 4096 | 4097, 256 m | 256 m + 1 entries), group 0 with the gadget, then the groups of _group_em_reference.chunk_case:
    exactly one chunk of 1024 rows, 1025 rows, one row; that case's other rows are in no group."""
    raw, cor, n = G.tier_case()
    raw2, cor2, n2 = G.chunk_case()
    k = G.TIER_K + GADGET_COLS
    assert raw2.shape[1] <= G.TIER_K
    raw2 = sp.csr_matrix((raw2.data, raw2.indices, raw2.indptr), shape=(raw2.shape[0], k))
    tier = sp.csr_matrix((raw.data, raw.indices, raw.indptr), shape=(raw.shape[0], k))
    both = sp.vstack([tier, raw2]).tocsr()
    cor = np.concatenate([cor, np.where(cor2 >= 0, cor2 + n, -1)]).astype(np.int32)
    rows = gadget_rows(G.TIER_K, int(both.max()))
    both, cor = _stack(both, cor, k, rows, [SPREAD_GADGET] * len(rows))
    case = Case('spread', both, cor, n + n2, 1, (SPREAD_GADGET,))
    assert case.class_counts() == (0, 0, 0, 0, n + n2)
    sizes = [len(case.group(n + i).rows) for i in range(3)]
    assert sizes == [G.SP_ROWS, G.SP_ROWS + 1, 1], sizes
    counts = sorted(set(int(x) for c in range(n) for x in case.group(c).n_col[case.group(c).cols]))
    for want in (32, 33, 64, 65, 192, 193, 4096, 4097, 256 * 17, 256 * 17 + 1):
        assert want in counts, (want, counts)
    assert all(x > 0 for x in case.spread_tiers())
    return case


@functools.lru_cache(maxsize=None)
def unique_only_case():
    """group 0: single-entry rows only (theta = 0 / 0 at theta_prior = 0); group 1: no rows; group 2: ordinary"""
    raw, _ = C.random_matrix(9, 120, 30, 1)
    lens = np.diff(raw.indptr)
    cor = np.full(raw.shape[0], -1, np.int32)
    uni = np.flatnonzero(lens == 1)
    cor[uni[:25]] = 0
    cor[np.flatnonzero(lens > 1)[:40]] = 2
    cor[uni[25:35]] = 2
    return raw, cor, 3


DEGENERATE = ('empty_rows', 'full_columns', 'K2', 'K1', 'unique_only')


@functools.lru_cache(maxsize=None)
def degenerate_case(key, spread):
    """the degenerate groups of the existing tests (rows without entries, Kc = 0, Kc = K, K = 1 and 2), a group of unique rows only
    and an empty group; one step each, in both classes — two for the group of unique rows only: the second starts from theta = NaN"""
    raw, cor, n = unique_only_case() if key == 'unique_only' else C.NAMED[key]()
    return Case('%s/%s' % (key, 'spread' if spread else 'one workgroup'), raw, cor, n, spread, (), T=2 if key == 'unique_only' else 1)


def case(name):
    return {'classes': classes_case, 'spread': spread_case}[name]()


# ---- trajectories on the CPU: the stop margins and the conditions on the inputs -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def trajectories(name, leg, order=LANE):
    """the emulation of every group of a case for T steps without a stop: [group][step]"""
    cs = case(name)
    _, pp, tp, use_lnl, _ = LEG[leg]
    return [emulate(g, (pp, tp), cs.T, 0.0, use_lnl, order) if len(g.rows) else [] for g in cs.groups()]


def _stop_steps(xs, eps):
    """per group the first step whose stop test holds (None: none within T)"""
    out = []
    for x in xs:
        hit = [t + 1 for t, v in enumerate(x) if v < eps]
        out.append(hit[0] if hit else None)
    return out


@functools.lru_cache(maxsize=None)
def leg_eps(name, leg):
    """The epsilon of a leg, from the CPU emulation alone: 0 for the leg that never stops; otherwise the candidate (a geometric mean
    of two neighbouring values of the stop tests' left sides over all groups and steps) with the widest gap around it among those
    under which one group at least stops before T and one does not — and, in the spread case, one group stops before, one at and
    one after the host's look after SP_LOOK iterations."""
    cs = case(name)
    if not LEG[leg][4]:
        return 0.0
    xs = [[s['x'] for s in tr] for tr in trajectories(name, leg)]
    vals = np.unique([v for x in xs for v in x if np.isfinite(v) and v > 0])
    # every left side stays a hundred times its own rounding noise away from epsilon (a step of pi: sum pi 2^-53 < 1e-14; a step of
    # lnl: about sqrt(terms) 2^-53 |lnl| < 1e-14 |lnl| of the group), so that another class's order of additions cannot move a stop
    noise = [1e-14 * (max([abs(s['lnl']) for s in tr if np.isfinite(s['lnl'])] + [1.0]) if LEG[leg][3] else 1.0) for tr in trajectories(name, leg)]
    best = None
    for a, b in zip(vals[:-1], vals[1:]):
        if any(abs(v - np.sqrt(a * b)) < 100 * nz for x, nz in zip(xs, noise) for v in x if np.isfinite(v)):
            continue
        eps = float(np.sqrt(a * b))
        stops = [t for t, x in zip(_stop_steps(xs, eps), xs) if x]
        early = [t for t in stops if t is not None and t < cs.T]
        if not early or len(early) == len(stops):
            continue
        if cs.spread and not (any(t < G.SP_LOOK for t in early) and G.SP_LOOK in early and any(t is not None and t > G.SP_LOOK for t in stops)):
            continue
        gap = b / a
        if best is None or gap > best[0]:
            best = (gap, eps)
    assert best is not None, (name, leg, 'no epsilon gives the stops the leg asks for')
    return best[1]


def stop_margin_failures(xs, eps):
    """the stop tests of a leg within 1e-6 relative of epsilon (fair_stops of _em_pass_reference)"""
    return E.fair_stops([v for x in xs for v in x if np.isfinite(v)], eps)
