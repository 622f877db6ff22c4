"""CPU: tests/_em_loop_reference.py is tied down without a GPU.

 1. `expected` (and the trace it reads) against OracleModel.em — n_iter, converged, and the trace's diff_t / lnl_t / parameters
    against the oracle's fp64 operator sequence — on golden cases and on the base matrix of tests/test_gpu_em_loop.py, at every
    placed stop, with and without use_likelihood, and for a second run seeded with the first run's lnl.
 2. `chunk_script` (which restates the contract of tsem_em_chunk from (n_iter, converged) alone) against a small model of the chunk
    loop that is driven by the VALUES of the trace, pass by pass, as the device is.
"""
import copy

import numpy as np
import pytest

import _em_loop_reference as L
from conftest import Opts, case_matrix, load_case

PRIORS = (0, 200000)
T_BASE = 16
STOPS = (1, 2, 3, 5, 8, 12)
_cache = {}


def base_matrix():
    from telescope_amd import synthetic
    if 'raw' not in _cache:
        m = synthetic.generate_csr(3000, 400, 6.0, seed=5, dist='zipf', uniq_frac=0.1)
        m.sort_indices()
        _cache['raw'] = m
    return _cache['raw']


def base_trace():
    if 'trace' not in _cache:
        _cache['trace'] = L.LoopTrace(base_matrix(), PRIORS, T_BASE)
    return _cache['trace']


def _oracle(raw, priors):
    from oracle.telescope_oracle import OracleModel
    return OracleModel(raw, *priors)


def test_base_matrix_is_what_the_stops_are_placed_on():
    """16 523 entries; every diff_est at least 1.3 x the next over 16 iterations, every |dlnl| at least 1.2 x the next up to
    iteration 12 (the smallest ratio is 1.248, iterations 3 / 4): the geometric mean of two neighbours lies a factor 1.09 from
    either, five orders above the 1e-6 fairness band, so a stop can be placed at every t of STOPS.  No undecided row at the
    iterations whose integer counts the GPU file compares."""
    raw, tr = base_matrix(), base_trace()
    assert raw.nnz == 16523 and raw.shape == (3000, 400)
    d = tr.deciding(False)
    assert np.all(d[1:-1] >= 1.3 * d[2:]), d
    l = tr.deciding(True)
    assert np.isinf(l[1]) and np.all(l[2:12] >= 1.2 * l[3:13]), l
    for t in STOPS + (T_BASE,):
        assert tr.undecided(t) == [], (t, tr.undecided(t))


def test_trace_against_the_oracle():
    """the trace's iterations against OracleModel (scipy's fp64 operator sequence): parameters, diff_est and lnl to 1e-12"""
    raw, tr = base_matrix(), base_trace()
    om = _oracle(raw, PRIORS)
    assert np.allclose(tr.stats, (om.total_wt, om.ambig_wt, om.weights.max()), rtol=1e-13, atol=0)
    assert np.allclose(tr.pisum0, np.asarray(om.pisum0).ravel(), rtol=1e-13, atol=0)
    steps = om.em(0.0, T_BASE, True)
    assert om.n_iter == T_BASE and not om.converged
    for t, (diff, lnl) in enumerate(steps, 1):
        assert abs(diff - tr.diff[t]) <= 1e-10 * tr.diff[t] + 1e-18, (t, diff, tr.diff[t])
        assert abs(lnl - tr.lnl[t]) <= 1e-12 * abs(tr.lnl[t]), (t, lnl, tr.lnl[t])
    assert np.allclose(om.pi, tr.pi[T_BASE], rtol=1e-11, atol=1e-300) and np.allclose(om.theta, tr.theta[T_BASE], rtol=1e-11, atol=1e-300)
    want = np.asarray(om.reassign('exclude').sum(0)).ravel()
    assert np.array_equal(tr.exclude_counts(T_BASE), want)


@pytest.mark.parametrize('use_likelihood', [False, True])
def test_expected_at_every_placed_stop(use_likelihood):
    raw, tr = base_matrix(), base_trace()
    for t in STOPS:
        if use_likelihood and t == 1:                             # |lnl_1 - inf| = inf on a fresh model: no epsilon stops there
            with pytest.raises(ValueError):
                L.eps_for_stop(tr, 1, True)
            continue
        eps = L.eps_for_stop(tr, t, use_likelihood)
        for max_iter in (T_BASE, t, max(1, t - 1)):
            om = _oracle(raw, PRIORS)
            om.em(eps, max_iter, use_likelihood)
            assert L.expected(tr, eps, use_likelihood, max_iter) == (om.n_iter, bool(om.converged)), (t, max_iter)
            if max_iter >= t:
                assert (om.n_iter, om.converged) == (t, True)
            if max_iter == T_BASE:
                assert np.array_equal(tr.exclude_counts(t), np.asarray(om.reassign('exclude').sum(0)).ravel()), t
    om = _oracle(raw, PRIORS)
    om.em(0.0, T_BASE, use_likelihood)
    assert L.expected(tr, 0.0, use_likelihood, T_BASE) == (T_BASE, False) == (om.n_iter, bool(om.converged))


def test_a_stop_that_cannot_be_placed_raises():
    tr = copy.copy(base_trace())
    tr.diff = tr.diff.copy()
    tr.diff[5] = 2.0 * tr.diff[3]                                # iteration 5 is not below every earlier one: an epsilon above it stops the run in 3
    with pytest.raises(ValueError):
        L.eps_for_stop(tr, 5, False)
    assert L.eps_for_stop(tr, 6, False) > tr.diff[6]
    with pytest.raises(ValueError):
        L.eps_for_stop(tr, 0, False)
    with pytest.raises(ValueError):
        L.eps_for_stop(tr, T_BASE + 1, False)


@pytest.mark.parametrize('t1', [3, 8])
def test_second_run_seeded_with_the_first_runs_lnl(t1):
    """model.py:786: the first lnl of a second em() is compared with what the first left"""
    raw, tr = base_matrix(), base_trace()
    eps = L.eps_for_stop(tr, t1, True)
    om = _oracle(raw, PRIORS)
    om.em(eps, T_BASE, True)
    assert (om.n_iter, om.converged) == (t1, True)
    tr2 = L.LoopTrace(raw, PRIORS, 6, start=(tr.pi[t1], tr.theta[t1]))
    om.em(eps, 6, True)
    assert L.expected(tr2, eps, True, 6, prev_lnl=tr.lnl[t1]) == (om.n_iter, bool(om.converged))
    assert om.n_iter == 1                                         # |lnl'_1 - lnl_t1| < eps: the changes only shrink
    # ... and placed in the second run itself
    for t2 in (1, 2, 3):
        try:
            e2 = L.eps_for_stop(tr2, t2, True, prev_lnl=tr.lnl[t1])
        except ValueError:
            continue
        om2 = _oracle(raw, PRIORS)
        om2.pi, om2.theta, om2.lnl = tr.pi[t1].copy(), tr.theta[t1].copy(), float(tr.lnl[t1])
        om2.em(e2, 6, True)
        assert L.expected(tr2, e2, True, 6, prev_lnl=tr.lnl[t1]) == (om2.n_iter, bool(om2.converged)) == (t2, True)


@pytest.mark.parametrize('name', ['bundled', 'bundled_lnl', 'tiny_one_row', 'tiny_empty_row', 'tiny_unique_only', 'tiny_twins', 'tiny_ties_lnl'])
def test_expected_on_golden_cases(name):
    c = load_case(name)
    raw = case_matrix(c).tocsr()
    o = Opts(c)
    use_lnl = bool(c['use_likelihood'])
    n_gold = int(c['n_iter'])
    T = min(o.max_iter, n_gold + 2)
    tr = L.LoopTrace(raw, (o.pi_prior, o.theta_prior), T)
    d = tr.deciding(use_lnl)
    import _em_pass_reference as E
    assert E.fair_stops(d[1:], o.em_epsilon, rel=L.FAIR_REL) == []
    max_iter = o.max_iter if bool(c['converged']) else T         # (an unconverged case: the same rules at a max_iter the trace reaches)
    got = L.expected(tr, o.em_epsilon, use_lnl, max_iter)
    om = _oracle(raw, (o.pi_prior, o.theta_prior))
    om.em(o.em_epsilon, max_iter, use_lnl)
    assert got == (om.n_iter, bool(om.converged))
    if bool(c['converged']):
        assert got == (n_gold, True)
        assert np.allclose(tr.pi[n_gold], c['pi'], rtol=1e-10, atol=0) and np.allclose(tr.theta[n_gold], c['theta'], rtol=1e-10, atol=0)


# ---- chunk_script against a value-driven model of the chunk loop ---------------------------------------------------------------------
def chunk_model(trace, eps, chunks, last_flags, scheme, prev_lnl=np.inf):
    """tsem_em_chunk pass by pass, on the trace's VALUES: what the kernels decide (k_update, k_lnl_check) and what the host copies out"""
    calls, inum, owing, prev, total = [], 0, False, prev_lnl, sum(chunks)
    for want, flush in zip(chunks, last_flags):
        done, stop, lnls, carry, owed_in = 0, False, [], None, owing
        for _ in range(want):
            t = inum + done + 1                                   # the iteration this pass would commit
            if scheme == L.LAGGED and owing:                      # its pass summed lnl_(t-1); its update tests that first
                l = trace.lnl[t - 1]
                hit, prev = abs(l - prev) < eps, l
                if done:
                    lnls[done - 1] = t - 1
                else:
                    carry = t - 1
                if hit:
                    stop, owing = True, False
                    break
            done += 1
            lnls.append(None)
            if scheme == L.DIFF:
                stop = trace.diff[t] < eps
            elif scheme == L.DEDICATED:
                l = trace.lnl[t]
                lnls[-1] = t
                stop, prev = abs(l - prev) < eps, l
            else:
                owing = True
            if stop:
                break
        if not stop and flush and scheme == L.LAGGED and owing:
            l = trace.lnl[inum + done]
            stop, prev, owing = abs(l - prev) < eps, l, False
            if done:
                lnls[done - 1] = inum + done
            else:
                carry = inum + done
        nan = () if scheme == L.DIFF else tuple(i for i, x in enumerate(lnls) if x is None)
        calls.append(dict(n_done=done, stopped=bool(stop), nan=nan, carry=carry if (owed_in and (done > 0 or not owing)) else None))
        inum += done
        if stop or inum >= total:
            break
    return calls


def chunkings(t, max_iter):
    """the chunkings of the GPU file, relative to a stop at t (None: never): one chunk, chunks of 1, t ends a chunk, t opens a chunk,
    chunks of 8 as tsem_em_run cuts"""
    out = {'one': (max_iter,), 'ones': (1,) * max_iter, 'eights': tuple(min(8, max_iter - i) for i in range(0, max_iter, 8))}
    if t is not None and t < max_iter:
        out['t_ends'] = (t, max_iter - t)
        if t > 1:
            out['t_opens'] = (t - 1, max_iter - t + 1)
        if t > 2:
            out['t_second'] = (t - 2, 3, max_iter - t - 1) if max_iter - t - 1 > 0 else (t - 2, max_iter - t + 2)
    return out


def test_chunk_script_against_the_model_of_the_loop():
    tr = base_trace()
    n = 0
    for scheme in L.SCHEMES:
        use_lnl = scheme != L.DIFF
        for t in STOPS + (None,):
            if t == 1 and use_lnl:
                continue
            eps = 0.0 if t is None else L.eps_for_stop(tr, t, use_lnl)
            for max_iter in sorted({T_BASE, t or T_BASE}):
                n_iter, conv = L.expected(tr, eps, use_lnl, max_iter)
                for key, chunks in chunkings(t, max_iter).items():
                    for flags in {tuple(L.flags_for(chunks)), (False,) * (len(chunks) - 1) + (True,)}:
                        want = chunk_model(tr, eps, chunks, flags, scheme)
                        got = L.chunk_script(chunks, flags, n_iter, conv, scheme)
                        assert L.script_of(got) == L.script_of(want), (scheme, t, max_iter, key, chunks, got, want)
                        assert sum(c['n_done'] for c in got) == n_iter and got[-1]['stopped'] == conv
                        n += 1
    assert n > 100


def test_chunk_script_names_the_cases_the_issue_places():
    """the three placements no earlier test reached, spelled out"""
    s = L.script_of
    # a stop by the owed lnl in the first pass of a later chunk: n_done = 0, stopped = 1, carry = lnl_t
    assert s(L.chunk_script((3, 5), (False, True), 3, True, L.LAGGED)) == [(3, False, (2,), None), (0, True, (), 3)]
    # a stop by the flush: max_iter == t
    assert s(L.chunk_script((3,), (True,), 3, True, L.LAGGED)) == [(3, True, (), None)]
    assert s(L.chunk_script((3,), (True,), 3, False, L.LAGGED)) == [(3, False, (), None)]
    # a stop seen inside the chunk: pass t + 1 lies in it
    assert s(L.chunk_script((2, 6), (False, True), 3, True, L.LAGGED)) == [(2, False, (1,), None), (1, True, (), 2)]
    # a stop in a chunk's last iteration under the other two schemes: counted at once, nothing carried
    for scheme in (L.DIFF, L.DEDICATED):
        assert s(L.chunk_script((3, 5), (False, True), 3, True, scheme)) == [(3, True, (), None)]
        assert s(L.chunk_script((1,) * 4, (False,) * 3 + (True,), 4, False, scheme)) == [(1, False, (), None)] * 4
    # chunks of 1, lagged: every call owes its lnl and brings the previous one
    assert s(L.chunk_script((1,) * 4, (False,) * 3 + (True,), 2, True, L.LAGGED)) == [(1, False, (0,), None), (1, False, (0,), 1), (0, True, (), 2)]
