"""A plain reference of the EM LOOP (model.py:762-806) and of the contract of tsem_em_chunk (include/telescope_em.h, the comment above
its declaration), for tests/test_em_loop_reference.py (CPU: this reference against OracleModel.em and against a small value-driven
model of the chunk loop) and tests/test_gpu_em_loop.py (GPU: tsem_em_chunk / tsem_em_run against this reference).

numpy only.  The iterations themselves come from tests/_em_pass_reference.py: exact (long double) column sums and log-likelihoods,
the closed forms of the M-step in fp64.  Nothing here touches the engine.

  LoopTrace       the loop at epsilon 0: pi_t, theta_t, diff_t, lnl_t for t = 1 .. T (index 0: the start parameters)
  expected        (n_iter, converged) of the reference's rules for an epsilon
  eps_for_stop    an epsilon that makes the run stop in iteration t, with a margin
  chunk_script    what every tsem_em_chunk call of a run returns besides the numbers: n_done, stopped, the NaN entries, the carry
"""
import numpy as np
import scipy.sparse as sp

import _em_pass_reference as E

LD = E.LD
DIFF, DEDICATED, LAGGED = 'diff', 'lnl_dedicated', 'lnl_lagged'
SCHEMES = (DIFF, DEDICATED, LAGGED)
FAIR_REL = 1e-6                                   # a stop test within 1e-6 of epsilon could go either way by rounding
UNDECIDED_RTOL = 1e-9                             # as tests/_bootstrap_reference.py: the two best z of a row within 1e-9 relative


def model_constants(raw, lut):
    """(stats, pisum0) of model.py:690-699 in fp64: stats = (total_wt, ambig_wt, the largest weight), w_i = max_j Q_ij;
    pisum0[j] = sum of Q_ij over the single-entry rows."""
    raw = sp.csr_matrix(raw)
    q = np.asarray(lut, dtype=np.float64)[raw.data]
    lens = np.diff(raw.indptr)
    rid = np.repeat(np.arange(raw.shape[0]), lens)
    w = np.zeros(raw.shape[0])
    np.maximum.at(w, rid, q)
    uni = (lens == 1)[rid]
    pisum0 = np.bincount(raw.indices[uni], weights=q[uni], minlength=raw.shape[1]).astype(np.float64)
    return (float(w.sum()), float(w[lens > 1].sum()), float(w.max(initial=0.0))), pisum0


class LoopTrace(object):
    """The reference loop at epsilon 0 for T iterations from `start` (None: pi = theta = 1 / K, model.py:667-673).
    pi[t], theta[t]: the parameters after iteration t (index 0: the start); diff[t] = sum |pi_t - pi_(t-1)| (model.py:781);
    lnl[t] = calculate_lnl(z(pi_(t-1), theta_(t-1)), pi_t, theta_t) (model.py:783); diff[0] = lnl[0] = NaN."""

    def __init__(self, raw, priors, T, start=None, lut=None):
        self.raw = raw = sp.csr_matrix(raw)
        raw.sort_indices()
        self.priors, self.T, self.K = tuple(priors), int(T), raw.shape[1]
        self.lut = E.lut(raw) if lut is None else np.asarray(lut, dtype=np.float64)
        self.stats, self.pisum0 = model_constants(raw, self.lut)
        a = (raw.indptr, raw.indices, raw.data, self.lut)
        k = self.K
        pi0, th0 = (np.full(k, 1.0 / k), np.full(k, 1.0 / k)) if start is None else (np.asarray(start[0], dtype=np.float64), np.asarray(start[1], dtype=np.float64))
        self.pi, self.theta = [pi0], [th0]
        self.diff, self.lnl = [np.nan], [np.nan]
        self.states = []                                        # RowState of the parameters an iteration STARTS from (z of its E-step)
        for _ in range(self.T):
            st = E.RowState(*a, self.pi[-1], self.theta[-1])
            why = E.fair(*a, self.pi[-1], self.theta[-1], state=st)
            assert why == [], why
            sums = E.exact_colsums(*a, self.pi[-1], self.theta[-1], state=st)[0]
            pi, theta, diff = E.exact_update(sums.astype(np.float64), self.pisum0, self.stats, self.priors, self.pi[-1])
            lnl = E.exact_lnl(*a, None, None, pi, theta, prev_state=st)[0]
            self.states.append(st)
            self.pi.append(pi); self.theta.append(theta)
            self.diff.append(float(diff)); self.lnl.append(float(lnl))
        self.diff, self.lnl = np.array(self.diff), np.array(self.lnl)

    def deciding(self, use_likelihood, prev_lnl=np.inf):
        """d[t], t = 1 .. T: what iteration t's stop test compares with epsilon — diff_t, or |lnl_t - lnl_(t-1)| with lnl_0 the lnl the
        previous run left (inf on a fresh model, model.py:683, 786).  d[0] = NaN."""
        if not use_likelihood:
            return self.diff.copy()
        with np.errstate(invalid='ignore'):
            l = np.concatenate([[prev_lnl], self.lnl[1:]])
            return np.concatenate([[np.nan], np.abs(l[1:] - l[:-1])])

    def undecided(self, t):
        """Rows whose assignment by the E-step of iteration t (z of pi_(t-1), theta_(t-1)) could go either way by rounding: the two
        best z within 1e-9 relative but not the same bits of the same product (equal Q and equal pi theta: a tie on both sides)."""
        st = self.states[t - 1]
        z = st.z.astype(np.float64)
        c = self.pi[t - 1] * self.theta[t - 1]                  # (rows of several entries: the numerators are Q pi theta)
        out = []
        ip = st.indptr
        for i in np.flatnonzero(st.lens > 1):
            v = z[ip[i]:ip[i + 1]]
            o = np.argsort(v, kind='stable')
            a, b = o[-1], o[-2]
            if v[a] - v[b] <= UNDECIDED_RTOL * v[a]:
                ja, jb = st.indices[ip[i] + a], st.indices[ip[i] + b]
                if not (st.q64[ip[i] + a] == st.q64[ip[i] + b] and c[ja] == c[jb]):
                    out.append(int(i))
        return out

    def exclude_counts(self, t):
        """Column sums of reassign('exclude') (model.py:837-842) on the z of iteration t's E-step: a row counts for its best column
        if that is the only best one.  Exact ties (the same bits) are ties; undecided(t) must be empty for the result to be used."""
        memo = self.__dict__.setdefault('_counts', {})
        if t in memo:
            return memo[t].copy()
        st = self.states[t - 1]
        z = st.z.astype(np.float64)
        out = np.zeros(self.K)
        ip = st.indptr
        for i in np.flatnonzero(st.lens > 0):
            v = z[ip[i]:ip[i + 1]]
            m = v.max()
            if m > 0 and np.count_nonzero(v == m) == 1:
                out[st.indices[ip[i] + int(np.argmax(v))]] += 1
        memo[t] = out
        return out.copy()


def expected(trace, eps, use_likelihood, max_iter, prev_lnl=np.inf):
    """(n_iter, converged) of model.py:771-797 over the trace: at least one iteration; iteration t ends the run when its test fires
    (diff_t < eps, or |lnl_t - lnl_(t-1)| < eps) or when t >= max_iter."""
    d = trace.deciding(use_likelihood, prev_lnl)
    t = 0
    while True:
        t += 1
        assert t <= trace.T, 'the trace ends before the run does'
        converged = bool(d[t] < eps)
        if converged or t >= max_iter:
            return t, converged


def eps_for_stop(trace, t, use_likelihood, prev_lnl=np.inf):
    """An epsilon with which the run stops in iteration t: the geometric mean of the deciding quantity at t and the smallest one
    before t (t = 1 has none before it: twice the deciding quantity).  Raises where no such epsilon exists — the deciding quantity
    at t is not below every earlier one, or is not finite — and asserts that no stop test of the trace lies within 1e-6 of it."""
    d = trace.deciding(use_likelihood, prev_lnl)
    if not (1 <= t <= trace.T) or not np.isfinite(d[t]) or d[t] <= 0:
        raise ValueError('no stop can be placed at iteration %d: its deciding quantity is %r' % (t, d[t] if 1 <= t <= trace.T else None))
    if t == 1:
        eps = 2.0 * d[1]
    else:
        before = float(np.min(d[1:t]))
        if not d[t] < before:
            raise ValueError('no stop can be placed at iteration %d: %r is not below the smallest earlier value %r' % (t, d[t], before))
        eps = float(np.sqrt(d[t] * before)) if np.isfinite(before) else 2.0 * d[t]
    assert E.fair_stops(d[1:], eps, rel=FAIR_REL) == [], ('a stop test within 1e-6 of epsilon', eps, d[1:])
    return eps


def chunk_script(chunks, last_flags, n_iter, converged, scheme):
    """The calls a host makes for a run that the reference ends after `n_iter` iterations (`converged`: by its stop test), cut into
    tsem_em_chunk calls of chunks[i] iterations at most with flags bit 1 = last_flags[i]; the host stops calling once a call says
    `stopped` or sum(chunks) iterations are committed.  One dict per call:
      n_done, stopped   the integers the call returns
      nan               the indices of lnls_out[0 .. n_done) that are NaN (always () under `diff`: no lnl is returned at all)
      carry             None: *lnl_carry is NaN; else the iteration whose lnl it is
      lnl_of            for every entry of lnls_out the iteration whose lnl it holds (None where NaN)
    The contract, restated (include/telescope_em.h):
      diff, lnl_dedicated   the test of iteration t runs in iteration t: n_done includes the stopping iteration; never a NaN, the
                            carry is always NaN.
      lnl_lagged            lnl_t is summed by the pass of iteration t+1 and tested by its update BEFORE it commits.  A chunk that
                            ends without a stop and without flushing returns its last lnl as NaN and owes it: the next call gives
                            it as the carry.  A stop in t is seen by pass t+1: when that pass lies in the same chunk, n_done counts
                            up to t; when t ended a chunk that did not flush, the next call returns n_done = 0, stopped = 1,
                            carry = lnl_t; a chunk that flushes tests its last lnl itself (dedicated pass) and returns it."""
    assert scheme in SCHEMES and len(chunks) == len(last_flags) and all(c >= 1 for c in chunks)
    total = sum(chunks)
    assert 1 <= n_iter <= total and (converged or n_iter == total)
    calls, inum, owed = [], 0, False
    for want, flush in zip(chunks, last_flags):
        owed_in = owed
        left = n_iter - inum
        if scheme != LAGGED:
            done = min(want, left)
            stop = converged and inum + done == n_iter
            nan, owed = (), False
        elif converged and left < want:                        # pass n_iter + 1 lies in this chunk
            done, stop, nan, owed = left, True, (), False
        else:
            assert left >= want
            done = want
            if flush:
                stop, nan, owed = converged and inum + done == n_iter, (), False
            else:
                stop, nan, owed = False, (done - 1,), True
        carry = inum if (scheme == LAGGED and owed_in and (done > 0 or not owed)) else None
        lnl_of = None if scheme == DIFF else [None if i in nan else inum + i + 1 for i in range(done)]
        calls.append(dict(n_done=done, stopped=bool(stop), nan=tuple(nan), carry=carry, lnl_of=lnl_of))
        inum += done
        if stop or inum >= total:
            break
    return calls


def drive(em_chunk, chunks, last_flags, eps, use_likelihood):
    """Run a sequence of em_chunk calls as a host does (first = the first call; stop after `stopped` or sum(chunks) iterations).
    em_chunk(n_max, eps, use_likelihood, first, last) -> (diffs, lnls or None, stopped, carry).  Returns (calls, diffs, lnls, n_iter,
    converged): per call what chunk_script describes, and the run's per-iteration values (lnls[t - 1] NaN where never delivered)."""
    total = sum(chunks)
    calls, diffs, lnls, inum, conv = [], [], [], 0, False
    for want, flush in zip(chunks, last_flags):
        d, l, stopped, carry = em_chunk(want, eps, use_likelihood, inum == 0, flush)
        nan = tuple(int(i) for i in np.flatnonzero(np.isnan(l))) if l is not None else ()
        calls.append(dict(n_done=len(d), stopped=bool(stopped), nan=nan, carry=None if np.isnan(carry) else inum))
        if not np.isnan(carry):
            assert inum > 0, 'a carry in the first call of a run'
            lnls[inum - 1] = float(carry)
        diffs.extend(float(x) for x in d)
        lnls.extend((float(x) for x in l) if l is not None else [np.nan] * len(d))
        inum += len(d)
        conv = bool(stopped)
        if conv or inum >= total:
            break
    return calls, np.array(diffs), np.array(lnls), inum, conv


def script_of(calls):
    """the comparable part of chunk_script's / drive's calls"""
    return [(c['n_done'], c['stopped'], c['nan'], c['carry']) for c in calls]


def flags_for(chunks):
    """flags bit 1 as tsem_em_run and em() set it: on the call that can reach max_iter = sum(chunks)"""
    total, inum, out = sum(chunks), 0, []
    for c in chunks:
        out.append(inum + c >= total)
        inum += c
    return out
