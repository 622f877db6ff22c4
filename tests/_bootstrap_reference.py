"""Reference for the bootstrap replicates (`TelescopeLikelihood.bootstrap`, tsem_bootstrap): replicate b gives row i a multiplicity
m_i, and its fit is BY DEFINITION the oracle's fit of the matrix in which row i appears m_i times, with the score scale of the whole
matrix.  Also the weighted closed form the device evaluates, in numpy (`weighted_fit`), so that the host tests can hold it against
that definition without a device.  Shared by tests/test_bootstrap_host.py and tests/test_gpu_bootstrap.py; every reference is computed
once per session and never changed."""
import functools
import warnings

import numpy as np
import scipy.sparse as sp

from _cell_em_reference import RTOL, random_matrix, twin_tie_matrix  # noqa: F401

EPSILON, MAX_ITER = 1e-7, 100
SEED, REPS = 7, (0, 1, 2, 3, 4)
METHODS = ('exclude', 'average', 'conf', 'unique', 'all')
INT_METHODS = ('exclude', 'unique', 'all')
CONF = 0.9
# case: (matrix seed, rows, K, pi_prior, theta_prior)
CASES = {'C1': (31, 3000, 200, 0, 200000), 'C2': (32, 2000, 50, 1, 5), 'C3': (33, 4000, 1500, 0, 200000), 'C4': (34, 1500, 40, 0, 0)}


@functools.lru_cache(maxsize=None)
def case_matrix(name):
    seed, n, k, _, _ = CASES[name]
    return random_matrix(seed, n, k, 1)[0]


def default_multiplicities(n_rows, seed=SEED, reps=REPS):
    from telescope_amd.synthetic import bootstrap_multiplicities
    return np.stack([bootstrap_multiplicities(seed, r, np.arange(n_rows)) for r in reps])


class BootRef(object):
    """The oracle's fit of every replicate: `fits[b]` is the OracleModel of `raw[np.repeat(arange(N), mult[b])]` (None where the
    replicate has no fragments), `fits[b].trace` its iterations' (diff, None)."""

    def __init__(self, raw, mult, pi_prior, theta_prior, epsilon=EPSILON, max_iter=MAX_ITER):
        from oracle.telescope_oracle import OracleModel
        self.raw, self.mult = sp.csr_matrix(raw), np.asarray(mult)
        self.N, self.K = self.raw.shape
        gmax = self.raw.max()
        self.fits = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                   # (theta = NaN at theta_prior = 0 divides 0 by 0, as the closed form says)
            for m in self.mult:
                rows = np.repeat(np.arange(self.N), m)
                if len(rows) == 0:
                    self.fits.append(None)
                    continue
                om = OracleModel(self.raw[rows], pi_prior, theta_prior, max_score=gmax)
                om.trace = om.em(epsilon, max_iter, False)
                self.fits.append(om)

    @functools.lru_cache(maxsize=None)
    def counts(self, b, method, thresh=CONF):
        """Column sums of the oracle's reassign(method) over the replicate's (repeated) rows = sum_i m_i A[i, j]."""
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return np.asarray(self.fits[b].reassign(method, thresh).sum(0)).ravel().astype(np.float64)

    @functools.lru_cache(maxsize=None)
    def undecided(self, conf_prob=CONF):
        """Rows of any replicate whose two largest z lie within RTOL relative of each other (twin columns of the twin matrix aside:
        see `twin_undecided`), or that have a z within RTOL of conf_prob: integer counts must not hinge on them."""
        out = 0
        for om in self.fits:
            if om is None or om.z is None:
                continue
            z = sp.csr_matrix(om.z)
            for i in range(z.shape[0]):
                v = z.data[z.indptr[i]:z.indptr[i + 1]]
                if len(v) == 0 or np.any(np.isnan(v)):
                    continue
                if np.any(np.abs(v - conf_prob) <= RTOL * conf_prob):
                    out += 1
                    continue
                if len(v) < 2:
                    continue
                s = np.sort(v)
                if s[-1] - s[-2] < RTOL * s[-1]:
                    out += 1
        return out

    def stop_margin(self, epsilon=EPSILON):
        """The smallest relative distance of any iteration's stop test of any replicate from epsilon."""
        worst = np.inf
        for om in self.fits:
            if om is None:
                continue
            for diff, _ in om.trace:
                if np.isfinite(diff):
                    worst = min(worst, abs(diff - epsilon) / epsilon)
        return worst


@functools.lru_cache(maxsize=None)
def case_ref(name):
    """The oracle's replicates 0..4 of seed 7 (default multiplicities) of a case, once per session."""
    _, _, _, pp, tp = CASES[name]
    raw = case_matrix(name)
    return BootRef(raw, default_multiplicities(raw.shape[0]), pp, tp)


def weighted_fit(raw, m, pi_prior, theta_prior, epsilon=EPSILON, max_iter=MAX_ITER, method='exclude', thresh=CONF):
    """The weighted closed form of one replicate in numpy — what the device unit computes: Q, Y, w of the WHOLE matrix, the
    replicate's W_tot = sum m w, W_amb = sum m w Y, w_max over the rows with m > 0, pisum0 = sum over unique rows of m Q; per
    iteration thetasum = sum m w z Y; lnl and the counts of `method` from the last E-step's z.  Returns a dict."""
    from telescope_amd.likelihood import score_lut
    raw = sp.csr_matrix(raw)
    n_rows, k = raw.shape
    m = np.asarray(m, dtype=np.float64)
    nan_k = np.full(k, np.nan)
    if m.sum() == 0:
        return dict(pi=nan_k, theta=nan_k, counts=nan_k, n_iter=0, converged=False, lnl=np.nan, n_frags=0)
    lut = score_lut(int(raw.max()))
    q = lut[raw.data]
    col = raw.indices
    lens = np.diff(raw.indptr)
    rid = np.repeat(np.arange(n_rows), lens)
    y = (lens > 1).astype(np.float64)
    w = np.zeros(n_rows)
    np.maximum.at(w, rid, q)
    tw, aw, wm = (m * w).sum(), (m * w * y).sum(), w[m > 0].max()
    ppw, tpw = pi_prior * wm, theta_prior * wm
    ps0 = np.bincount(col, weights=q * (1 - y[rid]) * m[rid], minlength=k)
    pi = np.full(k, 1. / k)
    th = pi.copy()

    def numer(p, t):
        return (q * y[rid]) * (p * t)[col] + (q * (1 - y[rid])) * p[col]

    def posterior(p, t):
        n = numer(p, t)
        rs = np.bincount(rid, weights=n, minlength=n_rows)
        with np.errstate(divide='ignore'):
            r = 1. / rs
        r[np.isinf(r)] = 0
        return n, n * r[rid]
    it, conv = 0, False
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        while True:
            pp, tp = pi, th
            n, z = posterior(pp, tp)
            s = np.bincount(col, weights=np.where(n != 0, (z * w[rid]) * y[rid], 0.) * m[rid], minlength=k)
            th = (s + tpw) / (aw + tpw * k)
            pi = ((ps0 + s) + ppw) / (tw + ppw * k)
            it += 1
            conv = bool(np.abs(pi - pp).sum() < epsilon)
            if conv or it >= max_iter:
                break
        n, z = posterior(pp, tp)
        n2 = numer(pi, th)
        keep = (n != 0) & (n2 != 0)
        lnl = float((m[rid][keep] * (z[keep] * np.log1p(n2[keep]))).sum())
        inp = n != 0
        zz = np.where(inp, z, -np.inf)
        zmax = np.full(n_rows, -np.inf)
        np.maximum.at(zmax, rid, zz)
        hole = (lens < k) | (np.bincount(rid, weights=~inp, minlength=n_rows) > 0)
        zmax = np.where(hole, np.maximum(zmax, 0.), zmax)
        best = inp & (z == zmax[rid])
        nbest = np.bincount(rid, weights=best, minlength=n_rows)
        if method == 'exclude':
            a = (best & (nbest[rid] == 1)).astype(float)
        elif method == 'average':
            a = best / np.where(nbest > 0, nbest, 1)[rid]
        elif method == 'conf':
            v = np.where(inp & (z >= thresh), z, 0.)
            cs = np.bincount(rid, weights=v, minlength=n_rows)
            a = v / np.where(cs > 0, cs, 1)[rid]
        elif method == 'unique':
            a = np.where(inp, np.ceil(z * (1 - y[rid])), 0.)
        elif method == 'all':
            a = (inp & (z > 0)).astype(float)
        else:
            raise ValueError(method)
        counts = np.bincount(col, weights=a * m[rid], minlength=k)
    if np.isnan(lnl):
        counts, lnl = nan_k, np.nan
    return dict(pi=pi, theta=th, counts=counts, n_iter=it, converged=conv, lnl=lnl, n_frags=int(m.sum()))


def check_replicates(fits, ref, label, params=True):
    """n_iter, converged, n_frags equal; pi, theta, lnl at RTOL (NaN where the oracle has NaN)."""
    assert fits.n_rep == len(ref.fits), label
    for b, om in enumerate(ref.fits):
        assert int(fits.n_frags[b]) == int(ref.mult[b].sum()), (label, b)
        if om is None:
            assert fits.n_iter[b] == 0 and not fits.converged[b] and np.isnan(fits.lnl[b]) and not fits.fitted[b], (label, b)
            assert np.all(np.isnan(fits.pi[b])) and np.all(np.isnan(fits.theta[b])) and np.all(np.isnan(fits.counts[b])), (label, b)
            continue
        assert int(fits.n_iter[b]) == om.n_iter and bool(fits.converged[b]) == bool(om.converged), \
            (label, b, int(fits.n_iter[b]), om.n_iter, bool(fits.converged[b]), om.converged)
        if params:
            for got, want, name in ((fits.pi[b], om.pi, 'pi'), (fits.theta[b], om.theta, 'theta')):
                assert np.allclose(got, want, rtol=RTOL, atol=0, equal_nan=True), (label, b, name, np.nanmax(np.abs(got / want - 1)))
            assert np.isclose(fits.lnl[b], om.lnl, rtol=RTOL, atol=0, equal_nan=True), (label, b, fits.lnl[b], om.lnl)
