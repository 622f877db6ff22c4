"""An exact reference of 1, 2 and 3 iterations of the bootstrap unit (telescope_amd/csrc/tsem_boot.hip: k_boot_sweep<0|1|2|3>,
k_boot_init, k_boot_update, k_boot_finish, the fold kernels), the rounding bounds the device is held to, and the seeded matrices and
multiplicities that tests/test_boot_pass_reference.py (CPU: this reference against `_bootstrap_reference.weighted_fit` and the
oracle) and tests/test_gpu_boot_pass_exact.py (GPU: the kernels against this reference) share.

numpy and np.longdouble only, in the style of tests/_em_pass_reference.py (its LD, U and the form of its bounds).  It is a reference
of the WEIGHTED CLOSED FORM — Q, Y, w of the whole matrix; W_tot = sum m w, W_amb = sum m w Y, w_max over the rows with m > 0,
pisum0 = sum over single-entry rows of m Q; per iteration thetasum = sum m w z Y — not of the oracle on repeated rows.  Nothing here
touches the engine.

THE BOUNDS.  Every addend of every sum of the sweeps is non-negative (Q = expm1(.) >= 0, parameters >= 0, m >= 0), so a sum of n
terms in ANY order — lanes, LDS accumulators, flushes, global atomics — has the relative error (n - 1) 2^-53 at most, first order.
All bounds are relative, first order, in units of U = 2^-53, functions of counts only; none was fitted to a device value.

  numerator   n = qa c + qu p with one of qa, qu exactly 0: one product.  The unit is compiled without FMA contraction; a contracted
              form would round once instead of twice — either form is allowed: 2.
  row sum     lane `sub` adds its ceil(len / 8) strided entries, sg_sum<8> adds three levels: ceil(len / 8) + 3 additions on top of
              the numerators' 2.
  reciprocal  1.
  term        v = (((n s) w) y) m: four products on top of n's 2 and s's (ceil(len / 8) + 3 + 2 + 1):
              term_own(len) = (ceil(len / 8) + 12) U.
  column sum  cnt_j - 1 additions of the replicate's live entries of column j:
              sum_own_j = (ceil(lenmax_j / 8) + cnt_j + 11) U.
  pisum0      m q (one product) and cnt0_j - 1 additions: cnt0_j U.
  W_tot, W_amb  m w (and y: exact) and the additions of the n_tot (n_amb) rows with m w > 0: n_tot U, n_amb U.
  theta_hat   (ts + tpw) / (W_amb + tpw K): tpw one product; numerator one addition; tpw K one product, the denominator's addition,
              the division: b_theta_j = b_ts_j + (n_amb + 6) U.  (Every part is non-negative: the relative error of a sum is at most
              the largest of its parts'.)
  pi_hat      ((ps0 + ts) + ppw) / (W_tot + ppw K): b_pi_j = max(cnt0_j U, b_ts_j) + (n_tot + 7) U.
  THE RECURRENCE.  After iteration t the device's parameters are not observable and differ from run to run (the atomics' order).
              With beta_c(t) = max_j (b_pi_j(t) + b_theta_j(t)) + U the bound of c = pi theta (one product) and beta_pi(t) that of
              pi, beta(t) = max(beta_c(t), beta_pi(t)): a z = n / S formed from parameters with relative error beta has the relative
              error 2 beta at most (beta in n, and beta in S, a positive combination of such n) plus the sweep's own:
                  b_ts_j(t) = 2 beta(t - 1) + sum_own_j,      beta(0) = 0 (pi = theta = fl(1 / K), c = fl(pi pi): the same bits).
              The constant is 2.
  diff        sum_j |pi_hat_j - pi_j|: K terms of one rounding each, added in any order, on top of the parameters' own bounds:
              sum_j (b_pi_j(t) pi_j(t) + b_pi_j(t - 1) pi_j(t - 1)) + (K + 1) U diff, absolute.
  z (last)    z_rel(len) = 2 beta(T - 1) + (ceil(len / 8) + 7) U (numerator 2, row sum, reciprocal, one product).
  lnl         sum m (z log1p(n2)): per term z_rel + (beta(T) + 2) U for n2 (d log1p(x) / log1p(x) <= dx / x) + 2 products, the
              logarithm within LNL_TERM max(1, log1p) as _em_pass_reference takes it, and (terms) U sum for the additions.
  counts      exclude, unique, all: integers below 2^53, exact.  average: 1 / best and the product with m, cnt - 1 additions:
              (cnt_j + 2) U.  conf: z / sum of the row's z >= thresh: 2 z_rel + (ceil(len / 8) + 3) + reciprocal + two products
              + cnt_j - 1 additions.
The group sink's values X_b of a slot are bounded like counts with the slot's own cnt.
"""
import numpy as np
import scipy.sparse as sp

import _em_pass_reference as E

LD = E.LD
U = E.U
LNL_TERM = E.LNL_TERM
METHODS = ('exclude', 'average', 'conf', 'unique', 'all')
INT_METHODS = ('exclude', 'unique', 'all')
CONF = 0.9
PRIORS = (0, 200000)
_sum_by, _max_by = E._sum_by, E._max_by


def _ceil8(lens):
    return (np.asarray(lens, dtype=np.int64) + 7) // 8


class Matrix(object):
    """What every replicate of one matrix shares: Q (fp64, the model's table at max_score = raw.max()), row lengths, Y, w, and the
    classes of twin columns (the same rows with the same scores: tsem_set_model's twin_rep)."""

    def __init__(self, raw, lut=None):
        raw = sp.csr_matrix(raw)
        raw.sort_indices()
        self.raw = raw
        self.N, self.K = raw.shape
        self.ip, self.col, self.data = raw.indptr.astype(np.int64), raw.indices.astype(np.int64), raw.data
        if lut is None:
            from telescope_amd.likelihood import score_lut
            lut = score_lut(int(raw.data.max()))
        self.lut = np.asarray(lut, dtype=np.float64)
        self.q64 = self.lut[self.data]
        self.q = self.q64.astype(LD)
        self.lens = np.diff(self.ip)
        self.rid = np.repeat(np.arange(self.N), self.lens)
        self.amb = self.lens > 1
        self.w = np.zeros(self.N)
        if len(self.rid):
            np.maximum.at(self.w, self.rid, self.q64)
        csc = sp.csc_matrix(raw)
        csc.sort_indices()
        seen, twin = {}, np.arange(self.K)
        for j in np.flatnonzero(np.diff(csc.indptr) > 0):
            a, b = csc.indptr[j], csc.indptr[j + 1]
            key = (csc.indices[a:b].tobytes(), csc.data[a:b].tobytes())
            twin[j] = seen.setdefault(key, j)
        self.twin = twin

    def row_sum(self, vals):
        out = np.zeros(self.N, dtype=LD)
        full = self.lens > 0
        if full.any():
            out[full] = np.add.reduceat(np.asarray(vals, dtype=LD), self.ip[:-1][full])
        return out

    def row_max(self, vals, empty):
        out = np.full(self.N, empty, dtype=LD)
        full = self.lens > 0
        if full.any():
            out[full] = np.maximum.reduceat(np.asarray(vals, dtype=LD), self.ip[:-1][full])
        return out


class Fit(object):
    """One replicate: see `fit`."""


def fit(M, m, priors=PRIORS, max_iter=1, eps=0.0, thresh=CONF, groups=None):
    """The weighted closed form of one replicate with multiplicities m[N] for at most `max_iter` iterations (stop: diff < eps), in
    long double, with its bounds.  Returns a Fit:
      n_frags, W_tot, W_amb, w_max, pisum0           the statistics (n_frags == 0: not fitted, NaN parameters, n_iter 0)
      pi[t], theta[t], b_pi[t], b_theta[t], t = 0..n_iter   parameters after iteration t and their relative bounds
      diff[t], b_diff[t] (absolute), t = 1..n_iter; n_iter, converged
      z, inpat, z_rel           the last E-step (from the parameters before the last M-step), per stored entry
      lnl, lnl_limit (absolute)
      counts[method], b_counts[method] (relative, per column)
      X[method], b_X[method] per slot of the (group, column) pattern where `groups` = (group_of_row, n_groups); slot_ptr, slot_cols"""
    f = Fit()
    K, N = M.K, M.N
    m = np.asarray(m).astype(np.int64)
    assert m.shape == (N,)
    f.m = m
    f.n_frags = int(m.sum())
    live = m > 0
    mL, wL = m.astype(LD), M.w.astype(LD)
    pp, tp = (LD(x) for x in priors)
    f.W_tot, f.W_amb = (mL * wL).sum(), (mL * wL)[M.amb].sum()
    f.w_max = float(M.w[live].max()) if live.any() else 0.0
    n_tot, n_amb = int((live & (M.w > 0)).sum()), int((live & (M.w > 0) & M.amb).sum())
    ppw, tpw = pp * LD(f.w_max), tp * LD(f.w_max)
    den_pi, den_th = f.W_tot + ppw * K, f.W_amb + tpw * K
    rid, col = M.rid, M.col
    me = mL[rid]
    uni = (~M.amb)[rid] & live[rid] & (M.q != 0)
    f.pisum0 = _sum_by(col[uni], (me * M.q)[uni], K)
    b_ps = np.bincount(col[uni], minlength=K).astype(LD) * LD(U)
    nan_k = np.full(K, np.nan)
    f.groups = groups
    if groups is not None:
        _pattern(M, f, groups)
    if f.n_frags == 0:
        f.n_iter, f.converged, f.lnl, f.lnl_limit = 0, False, np.nan, LD(0)
        f.pi, f.theta, f.b_pi, f.b_theta = [nan_k], [nan_k], [np.zeros(K, LD)], [np.zeros(K, LD)]
        f.diff, f.b_diff = [np.nan], [LD(0)]
        f.counts = {k: nan_k for k in METHODS}
        f.b_counts = {k: np.zeros(K, LD) for k in METHODS}
        f.z = f.inpat = f.z_rel = None
        if groups is not None:
            f.X = {k: np.full(len(f.slot_cols), np.nan) for k in METHODS}
            f.b_X = {k: np.zeros(len(f.slot_cols), LD) for k in METHODS}
        return f
    v = np.float64(1.0) / np.float64(K)
    c = np.full(K, np.float64(v * v)).astype(LD)              # k_boot_init: tab = (v v, v), the product rounded to fp64
    p = np.full(K, v).astype(LD)
    f.pi, f.theta = [p], [p.copy()]
    f.b_pi, f.b_theta = [np.zeros(K, LD)], [np.zeros(K, LD)]
    f.diff, f.b_diff, f.beta = [np.nan], [LD(0)], [LD(0)]
    amb_e = M.amb[rid]
    lens_e = M.lens[rid]
    t, conv = 0, False
    while True:
        c_prev, p_prev = c, p
        n, z, S = _estep(M, c_prev, p_prev)
        use = (n != 0) & amb_e & live[rid] & (z != 0)
        ts = _sum_by(col[use], (z * wL[rid] * me)[use], K)
        cnt = np.bincount(col[use], minlength=K).astype(LD)
        lenmax = _max_by(col[use], lens_e[use], K)
        own = np.where(cnt > 0, (_ceil8(lenmax).astype(LD) + cnt + 11) * LD(U), LD(0))
        b_ts = np.where(cnt > 0, 2 * f.beta[-1] + own, LD(0))
        with np.errstate(divide='ignore', invalid='ignore'):
            theta = (ts + tpw) / den_th
            pi = ((f.pisum0 + ts) + ppw) / den_pi
        b_theta = np.where(theta > 0, b_ts + (n_amb + 6) * LD(U), LD(0))
        b_pi = np.where(pi > 0, np.maximum(b_ps, b_ts) + (n_tot + 7) * LD(U), LD(0))
        diff = np.abs(pi - p_prev).sum()
        b_diff = (b_pi * pi + f.b_pi[-1] * p_prev).sum() + (K + 1) * LD(U) * diff
        beta = max(LD(np.max(b_pi + b_theta, initial=0)) + LD(U), LD(np.max(b_pi, initial=0)))
        t += 1
        f.pi.append(pi); f.theta.append(theta); f.b_pi.append(b_pi); f.b_theta.append(b_theta)
        f.diff.append(diff); f.b_diff.append(b_diff); f.beta.append(beta)
        c, p = pi * theta, pi
        conv = bool(diff < eps)
        if conv or t >= max_iter:
            break
    f.n_iter, f.converged = t, conv
    # ---- the last E-step again: z of (c_prev, p_prev), lnl against the final parameters ----
    inpat = n != 0
    f.z, f.inpat, f.S = z, inpat, S
    f.z_rel = 2 * f.beta[-2] + (_ceil8(lens_e).astype(LD) + 7) * LD(U)
    n2 = np.where(amb_e, M.q * c[col], M.q * p[col])
    keep = inpat & (n2 != 0) & live[rid]
    l = np.log1p(np.where(keep, n2, LD(0)))
    term = np.where(keep, me * z * l, LD(0))
    f.lnl = term.sum()
    nterm = int(np.count_nonzero(term))
    f.lnl_limit = (term * (f.z_rel + f.beta[-1] + 4 * LD(U))).sum() + LD(LNL_TERM) * np.where(keep, me * z * np.maximum(LD(1), l), LD(0)).sum() \
        + nterm * LD(U) * f.lnl
    # ---- reassign: the row maximum counts the zeros that are not stored (the `hole`), as _bootstrap_reference.weighted_fit ----
    zz = np.where(inpat, z, LD(-np.inf))
    zmax = M.row_max(zz, -np.inf)
    hole = (M.lens < K) | (M.row_sum((~inpat).astype(LD)) > 0)
    zmax = np.where(hole, np.maximum(zmax, LD(0)), zmax)
    f.zmax = zmax
    best = inpat & (z == zmax[rid])
    nbest = M.row_sum(best.astype(LD))
    above = inpat & (z >= LD(thresh))
    cs = M.row_sum(np.where(above, z, LD(0)))
    with np.errstate(divide='ignore', invalid='ignore'):
        a = {'exclude': (best & (nbest[rid] == 1)).astype(LD),
             'average': np.where(best, LD(1) / np.where(nbest > 0, nbest, LD(1))[rid], LD(0)),
             'conf': np.where(above, z / np.where(cs > 0, cs, LD(1))[rid], LD(0)),
             'unique': np.where(inpat, np.ceil(z * (~amb_e).astype(LD)), LD(0)),
             'all': (inpat & (z > 0)).astype(LD)}
    rel = {'exclude': 0, 'unique': 0, 'all': 0, 'average': 2 * LD(U),
           'conf': 2 * f.z_rel + (_ceil8(lens_e).astype(LD) + 6) * LD(U)}
    f.assign = a
    f.counts, f.b_counts = {}, {}
    for k in METHODS:
        on = live[rid] & (a[k] != 0)
        f.counts[k] = _sum_by(col[on], (a[k] * me)[on], K)
        f.b_counts[k] = _rel_bound(col[on], rel[k], on, K)
    if groups is not None:
        f.X, f.b_X = {}, {}
        for k in METHODS:
            on = live[rid] & (a[k] != 0) & (f.slot_of_entry >= 0)
            f.X[k] = _sum_by(f.slot_of_entry[on], (a[k] * me)[on], len(f.slot_cols))
            f.b_X[k] = _rel_bound(f.slot_of_entry[on], rel[k], on, len(f.slot_cols))
    return f


def _rel_bound(keys, rel, on, n):
    """per key: 0 for the integer methods; else the largest relative bound of its terms plus (cnt - 1) U for the additions"""
    if np.isscalar(rel) and rel == 0:
        return np.zeros(n, LD)
    r = np.broadcast_to(np.asarray(rel, dtype=LD), on.shape)[on]
    big = np.zeros(n, LD)
    if len(keys):
        np.maximum.at(big, keys, r)
    cnt = np.bincount(keys, minlength=n).astype(LD)
    return np.where(cnt > 0, big + cnt * LD(U), LD(0))


def _estep(M, c, p):
    n = np.where(M.amb[M.rid], M.q * c[M.col], M.q * p[M.col])
    S = M.row_sum(n)
    with np.errstate(divide='ignore', over='ignore'):
        ok = np.isfinite(1.0 / S.astype(np.float64))            # recip0: 1 / S = inf gives 0
    rinv = np.zeros(M.N, LD)
    rinv[ok] = LD(1) / S[ok]
    return n, n * rinv[M.rid], S


def _pattern(M, f, groups):
    """The pattern P of the group map: every stored (group, column), columns ascending within a group (tsem_cells.hip)."""
    grp, G = np.asarray(groups[0], dtype=np.int64), int(groups[1])
    ge = grp[M.rid]
    inside = (ge >= 0) & (ge < G)
    key = ge[inside] * M.K + M.col[inside]
    uniq = np.unique(key)
    f.slot_cols = (uniq % M.K).astype(np.int32)
    f.slot_ptr = np.searchsorted(uniq // M.K, np.arange(G + 1)).astype(np.int64)
    f.slot_of_entry = np.full(len(M.rid), -1, dtype=np.int64)
    f.slot_of_entry[inside] = np.searchsorted(uniq, key)


class BootPass(object):
    """The replicates of one call: fits[b] = fit(M, mult[b], ...) with one epsilon for all."""

    def __init__(self, raw, mult, priors=PRIORS, max_iter=1, eps=0.0, thresh=CONF, groups=None, M=None):
        self.M = M or Matrix(raw)
        self.mult = np.asarray(mult)
        self.priors, self.max_iter, self.eps, self.thresh = tuple(priors), int(max_iter), float(eps), thresh
        self.fits = [fit(self.M, m, priors, max_iter, eps, thresh, groups) for m in self.mult]

    def fair(self):
        return fair(self.M, self.fits, self.eps, self.thresh)


def fair(M, fits, eps=0.0, thresh=CONF):
    """The reasons, if any, why the input is no fair one for a comparison of integers; [] = fair.  ('row', replicate, row): a row
    whose integer decision is within the z bound of flipping — the best z against another z
    of the row, a z against `thresh`, z (1 - y) against 0 (a z that may underflow), a row sum so small that recip0 hangs on the
    order of the additions; ('stop', replicate, iteration): an iteration whose diff lies within its bound of eps.  Exact ties are not unfair: at
    n_iter = 1 the last z comes from pi = theta = 1 / K, so equal scores of one row give bit-equal z on the device; twin columns
    hold bit-equal parameters at any t (k_boot_update's twin_rep) and so bit-equal z for equal scores."""
    why = []
    for b, f in enumerate(fits):
        if f.n_frags == 0:
            continue
        for t in range(1, f.n_iter + 1):
            if eps > 0 and abs(f.diff[t] - LD(eps)) <= f.b_diff[t]:
                why.append(('stop', b, t))
        rid, z = M.rid, f.z
        on = f.inpat & (f.m > 0)[rid]
        # the entry that holds the row's best z
        order = np.lexsort((np.arange(len(z)), np.where(on, z, LD(-1)), rid))
        last = np.zeros(M.N, dtype=np.int64)
        last[rid[order]] = order                                  # (the last of a row in the order: its largest z)
        e1 = last[rid]
        z1 = z[e1]
        exact = (M.q64 == M.q64[e1]) & ((f.n_iter == 1) | (M.twin[M.col] == M.twin[M.col[e1]]))
        close = on & on[e1] & ~exact & (z1 - z <= 2 * f.z_rel * z1)
        edge = on & (np.abs(z - LD(thresh)) <= f.z_rel * z)
        tiny = on & (z < LD(E.TINY) * 4)
        low = np.zeros(len(z), dtype=bool)
        low[:] = ((f.S > 0) & (f.S < LD(2.0) ** -1020))[rid] & (f.m > 0)[rid]
        bad = np.unique(rid[close | edge | tiny | low])
        why.extend(('row', b, int(i)) for i in bad)
    return why


def eps_for_stop(diff, k):
    """An epsilon with which a replicate stops in iteration k and not before: the geometric mean of diff[k] and the smallest earlier
    diff (k = 1: twice diff[1]), at least 100 bounds away from both sides.  `diff`: a Fit (its diff[1 .. T] and their absolute
    bounds b_diff), or a pair (diff, b_diff) of sequences indexed from 1."""
    diff, b_diff = (diff.diff, diff.b_diff) if isinstance(diff, Fit) else diff
    d = [float(x) for x in diff]
    if not (1 <= k < len(d)) or not np.isfinite(d[k]) or d[k] <= 0:
        raise ValueError('no stop can be placed at iteration %d' % k)
    if k == 1:
        eps = 2.0 * d[1]
    else:
        before = min(d[1:k])
        if not d[k] < before:
            raise ValueError('no stop can be placed at iteration %d: %r is not below the smallest earlier value %r' % (k, d[k], before))
        eps = float(np.sqrt(d[k] * before))
    assert d[k] + 100 * float(b_diff[k]) < eps, ('the margin above diff[k]', d[k], float(b_diff[k]), eps)
    for t in range(1, k):
        assert d[t] - 100 * float(b_diff[t]) > eps, ('the margin below diff[%d]' % t, d[t], float(b_diff[t]), eps)
    return eps


def fraction(got, want, bound, absolute=False):
    """(largest |got - want| / limit, its index): limit = bound |want| (or the absolute `bound`); inf where the limit is 0 and the
    value differs (a zero is exact), or where exactly one side is NaN.  NaN on both sides counts as equal."""
    got = np.atleast_1d(np.asarray(got, dtype=np.float64))
    want = np.atleast_1d(np.asarray(want, dtype=LD))
    limit = np.broadcast_to(np.atleast_1d(np.asarray(bound, dtype=LD)), want.shape)
    if not absolute:
        limit = limit * np.abs(want)
    gn, wn = np.isnan(got), np.isnan(want.astype(np.float64))
    err = np.abs(got.astype(LD) - want)
    frac = np.zeros(len(want))
    ok = (limit > 0) & ~gn & ~wn
    frac[ok] = (err[ok] / limit[ok]).astype(np.float64)
    frac[~ok & ~gn & ~wn & (err > 0)] = np.inf
    frac[gn != wn] = np.inf
    j = int(np.argmax(frac)) if len(frac) else 0
    return (float(frac[j]) if len(frac) else 0.0), j


def welford(values, good):
    """mean and sd (ddof 1) of k_boot_fold / k_boot_fold_end in fp64, the replicates in order: d = x - mean; mean += d / k;
    M2 += d (x - mean).  values [n_rep x slots]; good [n_rep]."""
    values = np.asarray(values, dtype=np.float64)
    s = values.shape[1]
    mu, q, k = np.zeros(s), np.zeros(s), 0
    for b in range(values.shape[0]):
        if not good[b]:
            continue
        k += 1
        x = values[b]
        d = x - mu
        mu = mu + d / np.float64(k)
        q = q + d * (x - mu)
    mean = mu if k >= 1 else np.full(s, np.nan)
    with np.errstate(invalid='ignore'):
        sd = np.sqrt(q / np.float64(k - 1)) if k >= 2 else np.full(s, np.nan)
    return mean, sd, k


# ---- matrices and multiplicities both files use ------------------------------------------------------------------------------------
def _seed(*key):
    return E.R._seed('bootpass', *key)


def csr_from_rows(rows, k):
    """rows: a list of (columns, scores) per row; stored as given (explicit zeros are kept)"""
    lens = [len(c) for c, _ in rows]
    ip = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows] or [np.zeros(0, np.int32)])
    data = np.concatenate([np.asarray(s, dtype=np.uint16) for _, s in rows] or [np.zeros(0, np.uint16)])
    m = sp.csr_matrix((data, cols, ip), shape=(len(rows), k))
    m.sort_indices()
    return m


def random_rows(rng, n, k, lo=1, hi=40, uniq=0.25, cols=None, scores=(100, 400), hot=0, hot_share=0.0):
    """n rows of lo .. hi entries (a share `uniq` of one entry) over `cols` (default all k); a share `hot_share` of every row's entries
    falls on the first `hot` columns"""
    cols = np.arange(k) if cols is None else np.asarray(cols)
    out = []
    for _ in range(n):
        l = 1 if rng.rand() < uniq else int(rng.randint(max(lo, 2) if hi > 1 else 1, hi + 1))
        l = min(l, len(cols))
        nh = min(int(round(l * hot_share)), hot)
        pick = np.concatenate([rng.choice(hot, nh, replace=False), hot + rng.choice(len(cols) - hot, l - nh, replace=False)]) if hot else \
            rng.choice(len(cols), l, replace=False)
        c = np.sort(cols[pick.astype(np.int64)])
        out.append((c, rng.randint(scores[0], scores[1], l)))
    return out


def poisson_mult(rng, n_rep, n):
    return np.minimum(rng.poisson(1.0, (n_rep, n)), 255).astype(np.uint8)


# ---- the cases of the legs (tests/test_gpu_boot_pass_exact.py), built once ---------------------------------------------------------
N_A, K_A = 32 * 7 + 5, 60                         # leg a: 229 rows, 8 / 4 / 3 / 1 row ranges at 32 / 64 / 96 / 256 rows per workgroup
HOOKS = (32, 64, 96, 256, 8192)
ROW_LENGTHS = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255)
K_BIG = 65537 + 300                               # leg f: 258 update blocks, the last block's sum of diff_part takes a second trip
_cases = {}


class Case(object):
    def __init__(self, raw, mult, priors=PRIORS, groups=None, **note):
        self.raw, self.mult, self.priors, self.groups, self.note = raw, np.ascontiguousarray(mult, dtype=np.uint8), priors, groups, note
        self._M, self._refs = None, {}

    @property
    def M(self):
        if self._M is None:
            self._M = Matrix(self.raw)
        return self._M

    def ref(self, max_iter, eps=0.0, groups=None, reps=None):
        """the shared reference of (max_iter, eps, group map), computed once and never changed"""
        key = (max_iter, eps, None if groups is None else (groups[0].tobytes(), groups[1]), None if reps is None else tuple(reps))
        if key not in self._refs:
            mult = self.mult if reps is None else self.mult[list(reps)]
            self._refs[key] = BootPass(self.raw, mult, self.priors, max_iter, eps, groups=groups, M=self.M)
        return self._refs[key]


def _rows_a(n):
    rng = np.random.RandomState(_seed('a'))
    rows = random_rows(rng, 255, K_A, hi=40)
    return rows[:n], rng


def _case_a(n=N_A):
    """leg a (and g): rows of 1 - 40 entries over 60 columns, every column stored; 8 replicates of Poisson(1) draws with multiplicity 0
    planted on the whole first trips of some row ranges (rows 64 - 95 and 192 - 223)."""
    rows, rng = _rows_a(n)
    raw = csr_from_rows(rows, K_A)
    assert np.all(np.bincount(raw.indices, minlength=K_A) > 0)
    mult = poisson_mult(rng, 8, 255)[:, :n].copy()
    mult[:, 64:96] = 0
    mult[:, 192:224] = 0
    mult[:, n - 1] = np.maximum(mult[:, n - 1], 1)              # the last row of the last trip is live
    return Case(raw, mult)


def _case_b(cu):
    """leg b: the production formula gives 64 rows per workgroup on a device of `cu` compute units; rows of about 4 entries"""
    n, k = 128 * cu + 37, 300
    rng = np.random.RandomState(_seed('b', cu))
    lens = rng.randint(2, 7, n)
    lens[rng.rand(n) < 0.2] = 1
    m = E.R.matrix_from_lengths(lens, k, 300, rng, tie_scores=0.0)
    m.data = np.maximum(m.data, 100).astype(np.uint16)
    return Case(m, poisson_mult(rng, 8, n))


def _case_c():
    """leg c: every row length of ROW_LENGTHS three times among rows of 1 - 40 entries over 300 columns; empty rows first, in the
    middle and last; rows that store a score of 0 (Q = expm1(0) = 0 exactly: outside z's pattern, and they set `hole`)."""
    k = 300
    rng = np.random.RandomState(_seed('c'))
    rows = random_rows(rng, 400, k, hi=40)
    for l in ROW_LENGTHS * 3:
        c = np.sort(rng.choice(k, l, replace=False))
        rows.insert(int(rng.randint(0, len(rows))), (c, rng.randint(100, 400, l)))
    for _ in range(12):                                          # 3 - 12 entries, one or two of them with a stored score of 0
        l = int(rng.randint(3, 13))
        s = rng.randint(100, 400, l)
        s[rng.choice(l, int(rng.randint(1, 3)), replace=False)] = 0
        assert np.count_nonzero(s) >= 2
        rows.insert(int(rng.randint(0, len(rows))), (np.sort(rng.choice(k, l, replace=False)), s))
    empty = (np.zeros(0, np.int32), np.zeros(0, np.uint16))
    rows = [empty, empty] + rows[:200] + [empty] + rows[200:] + [empty]
    raw = csr_from_rows(rows, k)
    assert raw.data.min() == 0 and set(ROW_LENGTHS) <= set(np.diff(raw.indptr))
    return Case(raw, poisson_mult(rng, 5, raw.shape[0]))


def _case_full(k):
    """leg c: K = 8 / 9 with full rows (as many stored entries as columns: the `hole` is 0), one of them a tie of all its entries,
    among shorter rows"""
    rng = np.random.RandomState(_seed('full', k))
    rows = random_rows(rng, 90, k, hi=k, uniq=0.2)
    for _ in range(6):
        rows.insert(int(rng.randint(0, len(rows))), (np.arange(k), rng.randint(100, 400, k)))
    rows.insert(40, (np.arange(k), np.full(k, 250)))
    rows.append((np.arange(k), rng.randint(100, 400, k)))
    raw = csr_from_rows(rows, k)
    assert (np.diff(raw.indptr) == k).sum() >= 8
    return Case(raw, np.maximum(poisson_mult(rng, 4, raw.shape[0]), (np.diff(raw.indptr) == k).astype(np.uint8)), tie_row=40)


def _case_d300():
    """leg d (and e): 1500 rows of 1 - 40 entries over 300 columns, a third of every row's entries on the first 16 columns; in
    replicate 1 every row of the third most popular column drew 0; replicate 2 has 255 on every row of the fifth most popular one
    (`note`: zero_col, heavy_col)"""
    n, k = 1500, 300
    rng = np.random.RandomState(_seed('d300'))
    raw = csr_from_rows(random_rows(rng, n, k, hi=40, hot=16, hot_share=0.33), k)
    assert np.all(np.bincount(raw.indices, minlength=k) > 0)
    mult = poisson_mult(rng, 17, n)
    csc = raw.tocsc()
    order = np.lexsort((np.arange(k), -np.bincount(raw.indices, minlength=k)))      # most popular first, the lower id first among equals
    zero_col, heavy_col = int(order[2]), int(order[4])            # hot at any H >= 5
    mult[1, csc[:, zero_col].indices] = 0
    mult[2, csc[:, heavy_col].indices] = 255
    mult[4] = 0                                                  # a replicate of all zeros in the middle of a batch
    mult[6] = (np.diff(raw.indptr) == 1) * np.maximum(mult[6], 1)   # a replicate whose live rows are all unique
    mult[12] = 0                                                 # ... and one in the second batch
    return Case(raw, mult, zero_col=zero_col, heavy_col=heavy_col)


def _case_d6000():
    """leg d: H R at the cap of 5120 LDS accumulators: 6000 columns, every one stored"""
    n, k = 1500, 6000
    rng = np.random.RandomState(_seed('d6000'))
    rows = random_rows(rng, n, k, lo=8, hi=40, uniq=0.1)
    perm = rng.permutation(k)
    rows = [(np.unique(np.concatenate([c, perm[4 * i:4 * i + 4]])), None) for i, (c, _) in enumerate(rows)]
    rows = [(c, 100 + rng.choice(300, len(c), replace=False)) for c, _ in rows]   # (distinct scores in a row: columns that are twins in one replicate only cannot tie)
    raw = csr_from_rows(rows, k)
    assert np.all(np.bincount(raw.indices, minlength=k) > 0)
    return Case(raw, poisson_mult(rng, 8, n))


def _case_k(k):
    """leg f: K = 1, 2, 255, 256, 257; at 257 the columns 255 and 256 are twins (the same rows, the same scores) across the update
    kernel's block boundary"""
    n = 300
    rng = np.random.RandomState(_seed('k', k))
    if k == 257:
        rows = random_rows(rng, n, 256, hi=40)
        rows = [(np.concatenate([c, [256]]), np.concatenate([s, s[-1:]])) if c[-1] == 255 else (c, s) for c, s in rows]
        raw = csr_from_rows(rows, k)
        csc = raw.tocsc()
        assert csc[:, 255].nnz > 5 and (csc[:, 255] != csc[:, 256]).nnz == 0
    else:
        raw = csr_from_rows(random_rows(rng, n, k, hi=min(k, 40)), k)
    return Case(raw, poisson_mult(rng, 5, n))


def _case_kbig():
    """leg f: K = 65 837, 1000 rows; four fifths of the entries on the columns from 65 536 on (update blocks 256 and 257), so that
    most of diff comes from the part of the sum the last block's loop reaches in its second trip"""
    n, k = 1000, K_BIG
    rng = np.random.RandomState(_seed('kbig'))
    rows = []
    for _ in range(n):
        l = 1 if rng.rand() < 0.2 else int(rng.randint(2, 21))
        hi = int(np.ceil(l * 0.8))
        c = np.concatenate([65536 + rng.choice(k - 65536, hi, replace=False), rng.choice(200, l - hi, replace=False) * 300])
        rows.append((np.sort(c), rng.randint(100, 400, l)))
    return Case(csr_from_rows(rows, k), poisson_mult(rng, 3, n))


def case(name, *a):
    key = (name,) + a
    if key not in _cases:
        _cases[key] = {'a': _case_a, 'b': _case_b, 'c': _case_c, 'full': _case_full, 'd300': _case_d300, 'd6000': _case_d6000,
                       'k': _case_k, 'kbig': _case_kbig, 'stop': _case_stop}[name](*a)
    return _cases[key]


def group_maps(n):
    """leg g: (name, group_of_row, n_groups): every row a group of its own but the last 40 (in no group); one group of all rows; and
    three groups with rows in none between them"""
    one = np.arange(n, dtype=np.int32)
    one[n - 40:] = -1
    three = (np.arange(n) % 4).astype(np.int32) - 1
    return (('one_row', one, n - 40), ('all_rows', np.zeros(n, np.int32), 1), ('three', three, 3))


def kbig_eps(c):
    """leg f: an epsilon between iteration 2's diff and its part from the columns below 65 536 (what a sum of diff_part[0 .. 255]
    alone would give): the run goes on to iteration 3, a sum without the second trip stops in 2 — for every replicate, with 100
    bounds of margin on either side."""
    r = c.ref(3)
    lo, hi, bd = [], [], []
    for f in r.fits:
        d = np.abs(f.pi[2] - f.pi[1])
        lo.append(float(d[:65536].sum())); hi.append(float(d.sum())); bd.append(float(f.b_diff[2]))
        assert float(f.diff[1]) > float(f.diff[2])
    eps = float(np.sqrt(max(lo) * min(hi)))
    assert max(l + 100 * b for l, b in zip(lo, bd)) < eps < min(h - 100 * b for h, b in zip(hi, bd)), (lo, hi, bd)
    return eps


def _case_stop():
    """leg e: the matrix of d300 at pi_prior 1; replicate 2 lives on 3 rows and replicate 5 on 100, so that one epsilon (`stop_eps`)
    ends replicate 2 in iteration 1 and replicate 5 in iteration 2 while the six others run to max_iter = 3"""
    c = case('d300')
    n = c.raw.shape[0]
    rng = np.random.RandomState(_seed('stop'))
    mult = poisson_mult(rng, 8, n)
    for b, rows in ((2, 3), (5, 100)):
        mult[b] = 0
        mult[b, rng.choice(n, rows, replace=False)] = 1
    return Case(c.raw, mult, priors=(1, 200000))


def stop_eps(c):
    r = c.ref(3)
    f2, f5 = r.fits[2], r.fits[5]
    eps = eps_for_stop(f5, 2)
    assert float(f2.diff[1]) + 100 * float(f2.b_diff[1]) < eps
    for b, f in enumerate(r.fits):
        if b not in (2, 5):
            assert all(float(f.diff[t]) - 100 * float(f.b_diff[t]) > eps for t in (1, 2)), b
    return eps
