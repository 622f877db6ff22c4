"""`-m gpu`: the chunked EM loop — tsem_em_chunk / tsem_em_run, a state machine around the kernels — against tests/_em_loop_reference.py
(tied down without a GPU by tests/test_em_loop_reference.py): a stop placed ON PURPOSE at every position of a chunk, under the three
convergence schemes (the diff test in k_update; the dedicated lnl pass and k_lnl_check; the lagged lnl test of the MODE 4 pass), a
hand-off time-out injected at every position (options fused_dbg 32 / 64 with fused_dbg_skip), uneven row shards on the in-process
transport (empty ranks, a rank without ambiguous rows, a rank of one row), and k_local_reduce by itself.

Every leg asserts from layout_info that the layout and the lnl scheme it means to test were built, and prints `EMLOOP ...` lines
with the figures it asserts on (`pytest -s`); profiles/r24_em_loop.txt keeps a run.

Tolerances (those of tests/test_gpu_round4.py): lnl_t 1e-9 relative, diff_t rtol 1e-7 atol 1e-15, parameters 1e-9 relative.
Integers — n_iter, n_done, stopped, the NaN positions, the reassigned counts — exactly: every epsilon comes from
_em_loop_reference.eps_for_stop, which asserts that no stop test of the reference lies within 1e-6 of it, and the reference has no
undecided row at the iterations whose counts are compared (tests/test_em_loop_reference.py)."""
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import _em_loop_reference as L
from conftest import Opts, case_matrix, load_case

pytestmark = pytest.mark.gpu
PRIORS = (0, 200000)
T_BASE = 16
STOPS = (1, 2, 3, 5, 8, 12)
LNL_RTOL, PAR_RTOL, DIFF_RTOL, DIFF_ATOL = 1e-9, 1e-9, 1e-7, 1e-15
RENDEZVOUS_S = 20.0
_cache = {}
_faulted = []                                     # HIP errors / time-out codes met so far: after one, nothing more is started on the device
_worst = {'lnl': 0.0, 'par': 0.0, 'diff': 0.0}    # the largest errors of the file as fractions of their tolerances


def _say(fmt, *a):
    print('EMLOOP ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error or a time-out code (%s): no further work is started on the device' % _faulted[0])
    yield


def _track(eng):
    """the engine remembers a HIP error (TSEM_ERR_HIP) or a time-out code (TSEM_ERR_TIMEOUT) for the fixture above"""
    ck = eng._ck

    def _ck(rc):
        if rc in (-2, -4):
            _faulted.append('libtelescope_em error %d: %s' % (rc, eng._L.tsem_last_error(eng._h).decode()))
        ck(rc)
    eng._ck = _ck
    return eng


def base_matrix():
    from telescope_amd import synthetic
    if 'raw' not in _cache:
        m = synthetic.generate_csr(3000, 400, 6.0, seed=5, dist='zipf', uniq_frac=0.1)
        m.sort_indices()
        _cache['raw'] = m
    return _cache['raw']


def base_trace(raw=None, key='trace'):
    if key not in _cache:
        tr = L.LoopTrace(base_matrix() if raw is None else raw, PRIORS, T_BASE)
        for t in STOPS + (T_BASE,):
            assert tr.undecided(t) == [], ('an undecided row at iteration', t)
        _cache[key] = tr
    return _cache[key]


def _model(raw, options=(), comm=None, row_offset=0):
    """A TelescopeLikelihood over `raw` (this rank's rows) with engine options; the engine tracks faults."""
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood
    eng = _track(_lib.Engine(0))
    for key, v in options:
        eng.set_option(key, v)
    if row_offset:
        eng.set_option('row_offset', row_offset)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), raw.shape[1], None)    # (from_engine takes the global maximum and sets the table)
    return TelescopeLikelihood.from_engine(eng, Opts(pi_prior=PRIORS[0], theta_prior=PRIORS[1]), comm=comm)


def _frac(got, want, rtol, atol=0.0):
    """the largest |got - want| as a fraction of rtol |want| + atol (inf for a NaN, or a difference where the limit is 0)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0
    err, lim = np.abs(got - want), rtol * np.abs(want) + atol
    f = np.where(lim > 0, err / np.where(lim > 0, lim, 1.0), np.where(err > 0, np.inf, 0.0))
    f[np.isnan(got)] = np.inf
    return float(f.max())


def _scheme_built(info, scheme, options):
    """the layout and the lnl scheme a leg means to test, from layout_info"""
    o = dict(options)
    if o.get('em_kernel') == 1:
        assert info['fused'] == 0, info
    else:
        assert info['fused'] == 1 and info['nb'] > 0, info
    if o.get('value_format') == 1:
        assert info['value_bytes'] == 8 and info['split'] == 0, info
    if not o or 'use_likelihood' in o:
        assert info['value_bytes'] == 2 and info['split'] == 0, info
    if o.get('split') == 1:
        assert info['split'] == 1 and info['P'] == o['parts'], info
    if 'reproducible' in o:
        assert info['reproducible'] == 1, info
    if 'parts' in o:
        assert info['P'] == o['parts'], info
    assert info['lnl_fused'] == (1 if scheme == L.LAGGED else 0), (scheme, info)


def _start(tl, start=None, prev_lnl=np.inf):
    """the handle back at the start of a run: the start parameters (twice: previous = current) and the lnl the last run left"""
    k = tl.K
    pi, theta = (np.full(k, 1.0 / k), np.full(k, 1.0 / k)) if start is None else start
    tl._eng.set_params(pi, theta)
    tl._eng.set_params(pi, theta)
    tl._eng.set_prev_lnl(prev_lnl)


def _chunk_fn(eng, before_call=None):
    n = [0]

    def fn(n_max, eps, use_lnl, first, last):
        if before_call:
            before_call(n[0])
        n[0] += 1
        d, l, stopped = eng.em_chunk(n_max, eps, use_likelihood=use_lnl, first=first, last=last)
        return d, l, stopped, eng.lnl_carry
    return fn


def _check_values(tl, tr, n, diffs, lnls, use_lnl, label, counts=True):
    """what a run leaves: every diff_t and lnl_t against the trace, Z_CUR / Z_PREV / Z_FIRST = iterations n, n - 1 and 1, and the
    `exclude` counts of the last E-step"""
    from telescope_amd._lib import Z_CUR, Z_FIRST, Z_PREV
    assert len(diffs) == n, (label, len(diffs), n)
    fd = _frac(diffs, tr.diff[1:n + 1], DIFF_RTOL, DIFF_ATOL)
    assert fd <= 1.0, (label, 'diff_est', diffs, tr.diff[1:n + 1], fd)
    fl = 0.0
    if use_lnl:
        assert len(lnls) == n and not np.any(np.isnan(lnls)), (label, 'an lnl was never delivered', lnls)
        fl = _frac(lnls, tr.lnl[1:n + 1], LNL_RTOL)
        assert fl <= 1.0, (label, 'lnl', lnls, tr.lnl[1:n + 1], fl)
    fp = 0.0
    for which, t, name in ((Z_CUR, n, 'Z_CUR'), (Z_PREV, n - 1, 'Z_PREV'), (Z_FIRST, 1, 'Z_FIRST')):
        pi, theta = tl._eng.get_params(which)
        f = max(_frac(pi, tr.pi[t], PAR_RTOL), _frac(theta, tr.theta[t], PAR_RTOL))
        assert f <= 1.0, (label, name, 'is not iteration', t, f)
        fp = max(fp, f)
    if counts:
        tl._z, tl._z_which, tl._report_cache = None, Z_PREV, {}
        got = tl.reassign_colsums('exclude', 0.9, False)
        assert np.array_equal(got, tr.exclude_counts(n)), (label, 'exclude counts of the last E-step', np.flatnonzero(got != tr.exclude_counts(n))[:5])
    _worst['lnl'], _worst['par'], _worst['diff'] = max(_worst['lnl'], fl), max(_worst['par'], fp), max(_worst['diff'], fd)
    return fl, fp, fd


def _run(tl, tr, chunks, eps, scheme, max_iter, label, prev_lnl=np.inf, start=None, counts=True):
    """one run in em_chunk calls: the script of every call, n_iter / converged, the values"""
    use_lnl = scheme != L.DIFF
    flags = L.flags_for(chunks)
    want_n, want_c = L.expected(tr, eps, use_lnl, max_iter, prev_lnl)
    _start(tl, start, prev_lnl)
    calls, diffs, lnls, n, conv = L.drive(_chunk_fn(tl._eng), chunks, flags, eps, use_lnl)
    script = L.chunk_script(chunks, flags, want_n, want_c, scheme)
    assert L.script_of(calls) == L.script_of(script), (label, chunks, 'calls', L.script_of(calls), 'contract', L.script_of(script))
    assert (n, conv) == (want_n, want_c), (label, chunks, (n, conv), (want_n, want_c))
    f = _check_values(tl, tr, n, diffs, lnls, use_lnl, (label, chunks), counts)
    pi, theta = tl._eng.get_params()
    return dict(n=n, conv=conv, diffs=diffs, lnls=lnls, pi=pi, theta=theta, frac=f)


def chunkings(t, max_iter):
    """relative to a stop at t (None: never): one chunk of max_iter, chunks of 1, t ends a chunk, t opens a chunk"""
    out = {'one': (max_iter,), 'ones': (1,) * max_iter}
    if t is not None and t < max_iter:
        out['t_ends'] = (t, max_iter - t)
        if t > 1:
            out['t_opens'] = (t - 1, max_iter - t + 1)
    return out


def _bits(r):
    return tuple(np.asarray(r[k], dtype=np.float64).tobytes() for k in ('pi', 'theta', 'diffs', 'lnls'))


# ---- A. stop positions x chunkings x schemes, one engine ---------------------------------------------------------------------------
CODES, FP64, SPLIT, TWOPASS, REPRO = (), (('value_format', 1),), (('split', 1), ('parts', 5)), (('em_kernel', 1),), (('reproducible', 1),)
LEGS_A = [(L.DIFF, CODES), (L.DIFF, FP64), (L.DIFF, SPLIT), (L.DIFF, TWOPASS), (L.DIFF, REPRO),
          (L.DEDICATED, TWOPASS), (L.DEDICATED, FP64), (L.DEDICATED, REPRO), (L.LAGGED, (('use_likelihood', 1),)),
          (L.DIFF, (('parts', 4),)), (L.LAGGED, (('use_likelihood', 1), ('parts', 2)))]     # (teams of several workgroups: the exchange ring)


def _leg_name(leg):
    return leg[0] + '-' + ('-'.join('%s%d' % kv for kv in leg[1]) or 'codes')


@pytest.mark.parametrize('leg', LEGS_A, ids=_leg_name)
def test_stop_at_every_position(gpu_device, leg):
    """A stop at t in 1, 2, 3, 5, 8, 12 and never, under one chunk of max_iter, chunks of 1, t ending a chunk, t opening a chunk,
    max_iter == t (the last chunk's flush decides under the lagged scheme) and chunks of 8 through tsem_em_run: per call the
    contract (chunk_script) exactly, per run n_iter / converged, every lnl_t and diff_t, the three parameter sets and the counts of
    the last E-step.  With option "reproducible" every chunking of one epsilon gives the same bits."""
    scheme, options = leg
    use_lnl = scheme != L.DIFF
    tr = base_trace()
    tl = _model(base_matrix(), options)
    eng = tl._eng
    _scheme_built(eng.layout_info(), scheme, options)
    runs, top = 0, [0.0, 0.0, 0.0]
    for t in STOPS + (None,):
        if t == 1 and use_lnl:
            continue                                                # |lnl_1 - inf| on a fresh model: no epsilon stops there (the second run below does)
        eps = 0.0 if t is None else L.eps_for_stop(tr, t, use_lnl)
        same = []
        for max_iter in sorted({T_BASE, t or T_BASE}):
            for key, chunks in chunkings(t, max_iter).items():
                r = _run(tl, tr, chunks, eps, scheme, max_iter, '%s stop %s %s' % (_leg_name(leg), t, key))
                assert (r['n'], r['conv']) == ((t, True) if t else (T_BASE, False))
                same.append((key, max_iter, r))
                top = [max(a, b) for a, b in zip(top, r['frac'])]
                runs += 1
            # chunks of 8, as tsem_em_run cuts, through Engine.em_run itself
            _start(tl)
            res = eng.em_run(eps, max_iter, use_lnl)
            want = L.expected(tr, eps, use_lnl, max_iter)
            assert (res['n_iter'], res['converged']) == want, ('em_run', t, max_iter, res['n_iter'], res['converged'], want)
            f = _check_values(tl, tr, res['n_iter'], res['diffs'], res['lnls'], use_lnl, ('em_run', t, max_iter))
            assert _frac(res['lnl'], tr.lnl[res['n_iter']], LNL_RTOL) <= 1.0, ('em_run: the final lnl', res['lnl'], tr.lnl[res['n_iter']])
            assert max(_frac(res['pi_init'], tr.pi[1], PAR_RTOL), _frac(res['theta_init'], tr.theta[1], PAR_RTOL)) <= 1.0
            pi, theta = eng.get_params()
            same.append(('em_run', max_iter, dict(pi=pi, theta=theta, diffs=res['diffs'], lnls=res['lnls'] if use_lnl else np.full(res['n_iter'], np.nan))))
            top = [max(a, b) for a, b in zip(top, f)]
            runs += 1
        if 'reproducible' in dict(options):
            first = _bits(same[0][2])
            for key, max_iter, r in same[1:]:
                assert _bits(r) == first, ('option reproducible: chunking', key, max_iter, 'gives other bits than', same[0][0], 'at stop', t)
    info = eng.layout_info()
    assert info['fallbacks'] == 0, info
    _say('%s: %d runs; largest lnl error %.3g, parameter error %.3g, diff error %.3g of their tolerances; P %d R %d nb %d', _leg_name(leg), runs,
         top[0], top[1], top[2], info['P'], info['R'], info['nb'])


@pytest.mark.parametrize('leg', [(L.LAGGED, (('use_likelihood', 1),)), (L.DEDICATED, TWOPASS), (L.DEDICATED, FP64)], ids=_leg_name)
def test_second_run_on_the_same_handle(gpu_device, leg):
    """model.py:786: a second run (`first` again) compares its first lnl with the lnl the first run left — kept by tsem_em_run, or
    set through set_prev_lnl — and stops where expected(..., prev_lnl = lnl of run 1) says: in iteration 1 with the first run's
    epsilon, and at placed stops of its own trace."""
    scheme, options = leg
    tr = base_trace()
    tl = _model(base_matrix(), options)
    eng = tl._eng
    _scheme_built(eng.layout_info(), scheme, options)
    for t1 in (3, 8):
        eps = L.eps_for_stop(tr, t1, True)
        start2 = (tr.pi[t1], tr.theta[t1])
        key = ('trace2', t1)
        if key not in _cache:
            _cache[key] = L.LoopTrace(base_matrix(), PRIORS, 6, start=start2)
        tr2 = _cache[key]
        # tsem_em_run twice: the second run starts from the device's own state and the lnl it kept
        _start(tl)
        r1 = eng.em_run(eps, T_BASE, True)
        assert (r1['n_iter'], r1['converged']) == (t1, True)
        r2 = eng.em_run(eps, 6, True)
        want = L.expected(tr2, eps, True, 6, prev_lnl=tr.lnl[t1])
        assert want == (1, True) and (r2['n_iter'], r2['converged']) == want, (t1, r2['n_iter'], r2['converged'], want)
        _check_values(tl, tr2, 1, r2['diffs'], r2['lnls'], True, ('second em_run', t1), counts=False)
        # em_chunk with set_prev_lnl, stops placed in the second run's own trace
        placed = 0
        for t2 in (1, 2, 3):
            try:
                e2 = L.eps_for_stop(tr2, t2, True, prev_lnl=tr.lnl[t1])
            except ValueError:
                continue
            for chunks in ((6,), (1,) * 6, (t2, 6 - t2)):
                r = _run(tl, tr2, chunks, e2, scheme, 6, 'second run after %d, stop %d' % (t1, t2), prev_lnl=float(tr.lnl[t1]), start=start2, counts=False)
                assert (r['n'], r['conv']) == (t2, True)
            placed += 1
        assert placed >= 2, 'the second run\'s trace allows fewer than two placed stops'
    assert eng.layout_info()['fallbacks'] == 0


# ---- B. time-outs at every position ------------------------------------------------------------------------------------------------
B_CHUNKS = (6, 4, 6)
# (scheme, options, bit, arm before call, skip, stop)
LAG_OPT = (('use_likelihood', 1),)
LEGS_B = [
    (L.DIFF, CODES, 32, 0, 0, None),                # iteration 1 of a `first` chunk: Z_FIRST must come from the redone iteration
    (L.DIFF, CODES, 32, 0, 1, None), (L.DIFF, CODES, 32, 0, 3, None),
    (L.DIFF, CODES, 32, 1, 3, None),                # the last iteration of a chunk
    (L.DIFF, CODES, 32, 0, 3, 4),                   # the pass that would have found the run converged
    (L.DIFF, CODES, 32, 0, 0, 1),                   # ... in iteration 1
    (L.DIFF, SPLIT, 32, 0, 3, None),                # (split: two launches per pass)
    (L.DIFF, REPRO, 32, 0, 0, None), (L.DIFF, REPRO, 32, 0, 3, 4),
    (L.DEDICATED, CODES, 32, 0, 0, None), (L.DEDICATED, CODES, 32, 0, 3, 4),
    (L.DEDICATED, CODES, 64, 0, 0, None), (L.DEDICATED, CODES, 64, 0, 1, None), (L.DEDICATED, CODES, 64, 0, 3, None),
    (L.DEDICATED, CODES, 64, 1, 3, None),           # the lnl pass of a chunk's last iteration
    (L.DEDICATED, CODES, 64, 0, 3, 4),              # the lnl pass that would have found the run converged
    (L.DEDICATED, REPRO, 64, 0, 1, 4),
    (L.LAGGED, LAG_OPT, 32, 0, 0, None),          # iteration 1 of a `first` chunk
    (L.LAGGED, LAG_OPT, 32, 0, 1, None),          # inside a chunk, an lnl owed by the iteration committed just before (ctl[1] > 0)
    (L.LAGGED, LAG_OPT, 32, 0, 3, None),
    (L.LAGGED, LAG_OPT, 32, 1, 0, None),          # the first pass of a later chunk while an lnl is owed (ctl[1] == 0)
    (L.LAGGED, LAG_OPT, 32, 1, 3, None),          # the last iteration of a chunk
    (L.LAGGED, LAG_OPT, 32, 0, 3, 3),             # pass 4 would have found the run converged in 3
    (L.LAGGED, LAG_OPT, 32, 1, 0, 6),             # ... and so would the first pass of the next chunk: the owed lnl ends the run
    (L.LAGGED, LAG_OPT, 64, 0, 0, None),          # the flush of the last chunk is an lnl pass
]


def _b_name(leg):
    return '%s-%s-bit%d-call%d-skip%d-stop%s' % (leg[0], '-'.join('%s%d' % kv for kv in leg[1]) or 'codes', leg[2], leg[3], leg[4], leg[5])


@pytest.mark.parametrize('leg', LEGS_B, ids=_b_name)
def test_timeout_at_every_position(gpu_device, leg):
    """The fused EM pass (fused_dbg 32) or lnl pass (64) behaves like a hand-off time-out after `skip` launches of its kind, armed
    before a given call of a run in chunks of 6 + 4 + 6: the trace, n_iter, converged and the three parameter sets are those of the
    run without a time-out, Z_FIRST is iteration 1, every iteration's lnl is delivered exactly once (in lnls_out or as a carry),
    one fall-back — and with option "reproducible" the handle stays fused and gives the bits of an undisturbed run."""
    scheme, options, bit, arm, skip, stop = leg
    use_lnl = scheme != L.DIFF
    repro = 'reproducible' in dict(options)
    tr = base_trace()
    eps = 0.0 if stop is None else L.eps_for_stop(tr, stop, use_lnl)
    max_iter = sum(B_CHUNKS)
    want = L.expected(tr, eps, use_lnl, max_iter)
    flags = L.flags_for(B_CHUNKS)
    label = _b_name(leg)
    tl = _model(base_matrix(), options)
    eng = tl._eng
    _scheme_built(eng.layout_info(), scheme, options)
    clean = None
    if repro:
        clean = _run(tl, tr, B_CHUNKS, eps, scheme, max_iter, label + ' (undisturbed)')

    def arm_it(call):
        if call == arm:
            eng.set_option('fused_dbg', bit)
            eng.set_option('fused_dbg_skip', skip)
    _start(tl)
    delivered = np.zeros(max_iter + 1, dtype=np.int64)
    fn = _chunk_fn(eng, arm_it)
    seen = [0]

    def counting(n_max, eps_, ul, first, last):
        d, l, stopped, carry = fn(n_max, eps_, ul, first, last)
        if l is not None:
            for i, x in enumerate(l):
                if not np.isnan(x):
                    delivered[seen[0] + i + 1] += 1
        if not np.isnan(carry):
            delivered[seen[0]] += 1
        seen[0] += len(d)
        return d, l, stopped, carry
    calls, diffs, lnls, n, conv = L.drive(counting, B_CHUNKS, flags, eps, use_lnl)
    info = eng.layout_info()
    assert (n, conv) == want, (label, (n, conv), want, L.script_of(calls))
    if use_lnl:
        assert np.array_equal(delivered[1:n + 1], np.ones(n, dtype=np.int64)) and delivered[0] == 0 and not delivered[n + 1:].any(), \
            (label, 'every lnl exactly once', delivered, L.script_of(calls))
    f = _check_values(tl, tr, n, diffs, lnls, use_lnl, label)
    if scheme != L.LAGGED:                                      # (the lagged scheme ends at the time-out: from there on the dedicated pass runs)
        script = L.chunk_script(B_CHUNKS, flags, want[0], want[1], scheme)
        assert L.script_of(calls) == L.script_of(script), (label, L.script_of(calls), L.script_of(script))
    else:
        # up to the call of the time-out the lagged contract, afterwards no NaN and no further carry than the one owed at the time-out
        script = L.chunk_script(B_CHUNKS, flags, want[0], want[1], L.LAGGED)
        first_hit = arm if bit == 32 else len(calls) - 1
        assert L.script_of(calls[:first_hit]) == L.script_of(script[:first_hit]), (label, L.script_of(calls), L.script_of(script))
        for c in calls[first_hit:]:
            assert c['nan'] == (), (label, 'a NaN after the fall-back', L.script_of(calls))
        assert all(c['carry'] is None for c in calls[first_hit + 1:]), (label, 'a carry after the fall-back', L.script_of(calls))
    assert info['fallbacks'] == 1, (label, info)
    if repro:
        assert info['fused'] == 1 and info['reproducible'] == 1, (label, info)
        pi, theta = eng.get_params()
        assert _bits(dict(pi=pi, theta=theta, diffs=diffs, lnls=lnls)) == _bits(clean), (label, 'the bits of the undisturbed run')
    else:
        assert info['fused'] == 0, (label, info)
    _say('%s: n_iter %d converged %d; calls %s; lnl %.3g par %.3g diff %.3g of their tolerances', label, n, conv, L.script_of(calls), *f)


# ---- C. uneven shards on the in-process transport ----------------------------------------------------------------------------------
def _run_ranks(world, fn, barrier=None):
    """fn(rank) on `world` host threads; re-raises the first failure (the group's rendezvous time-out and the aborted host barrier
    end the other ranks)"""
    out, errs = [None] * world, []

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:   # noqa: BLE001
            errs.append((r, e))
            if barrier is not None:
                barrier.abort()
    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(300) for t in ts]
    if any(t.is_alive() for t in ts):
        _faulted.append('a rank hangs')
    assert not any(t.is_alive() for t in ts), 'a rank hangs'
    if errs:
        first = [e for e in errs if 'did not reach the collective' not in str(e[1]) and 'BrokenBarrier' not in type(e[1]).__name__] or errs
        raise first[0][1]
    return out


def seam_matrix():
    """vstack(rows with several entries, rows with one entry) of the base matrix"""
    if 'seam' not in _cache:
        raw = base_matrix()
        lens = np.diff(raw.indptr)
        m = sp.vstack([raw[np.flatnonzero(lens > 1)], raw[np.flatnonzero(lens == 1)], raw[np.flatnonzero(lens == 0)]]).tocsr()
        m.sort_indices()
        _cache['seam'] = (m, int((lens > 1).sum()))
    return _cache['seam']


def _cuts(name):
    """(matrix, trace key, row cuts, can every rank carry the lnl)"""
    raw = base_matrix()
    n = raw.shape[0]
    if name == 'w2_rank1_empty':
        return raw, 'trace', [0, n, n], False
    if name == 'w2_rank0_empty':
        return raw, 'trace', [0, 0, n], False
    if name == 'w3_middle_empty':
        return raw, 'trace', [0, 1400, 1400, n], False
    if name == 'w3_seam':
        m, n_amb = seam_matrix()
        return m, 'trace_seam', [0, n_amb // 2, n_amb, m.shape[0]], False
    if name == 'w4_one_row':
        assert np.diff(raw.indptr)[0] > 1                        # (rank 0 holds row 0 alone, a row of several entries: it can carry the lnl)
        return raw, 'trace', [0, 1, 1000, 2000, n], True
    raise KeyError(name)


def _single_reference(raw, key, eps, use_lnl, max_iter, seed):
    """the single-engine run of the same matrix: exclude / choose / conf column sums"""
    ck = ('single', key, eps, use_lnl, max_iter)
    if ck not in _cache:
        tl = _model(raw, (('use_likelihood', 1),) if use_lnl else ())
        _start(tl)
        res = tl._eng.em_run(eps, max_iter, use_lnl)
        from telescope_amd._lib import Z_PREV
        tl._z, tl._z_which, tl._report_cache = None, Z_PREV, {}
        np.random.seed(seed)
        out = dict(n_iter=res['n_iter'], choose=tl.reassign_colsums('choose', 0.9, False), exclude=tl.reassign_colsums('exclude', 0.9, False),
                   conf=tl.reassign_colsums('conf', 0.9, False))
        _cache[ck] = out
    return _cache[ck]


def _sharded(raw, tr, cuts, chunks, eps, use_lnl, label, seed=7, timeout_rank=None):
    from telescope_amd.distributed import ThreadGroup
    from telescope_amd._lib import Z_PREV
    world = len(cuts) - 1
    group = ThreadGroup(0, world)
    group.set_timeout(RENDEZVOUS_S)
    flags = L.flags_for(chunks)
    options = (('use_likelihood', 1),) if use_lnl else ()

    def rank_main(rank):
        comm = group.comm(rank)
        try:
            r0, r1 = cuts[rank], cuts[rank + 1]
            tl = _model(raw[r0:r1], options, comm=comm, row_offset=r0)
            eng = tl._eng
            info0 = eng.layout_info()
            if timeout_rank == rank:
                eng.set_option('fused_dbg', 32)
                eng.set_option('fused_dbg_skip', 1)
            _start(tl)
            calls, diffs, lnls, n, conv = L.drive(_chunk_fn(eng), chunks, flags, eps, use_lnl)
            f = _check_values(tl, tr, n, diffs, lnls, use_lnl, (label, 'rank', rank), counts=False)
            pi, theta = eng.get_params()
            tl._z, tl._z_which, tl._report_cache = None, Z_PREV, {}
            if rank == 0:
                np.random.seed(seed)
            res = dict(calls=L.script_of(calls), n=n, conv=conv, diffs=diffs, lnls=lnls, pi=pi, theta=theta, frac=f, info0=info0,
                       choose=tl.reassign_colsums('choose', 0.9, False), exclude=tl.reassign_colsums('exclude', 0.9, False),
                       conf=tl.reassign_colsums('conf', 0.9, False), info=eng.layout_info())
            return res
        finally:
            comm.close()
    try:
        return _run_ranks(world, rank_main, group.barrier)
    finally:
        group.close()


@pytest.mark.parametrize('cut', ['w2_rank1_empty', 'w2_rank0_empty', 'w3_middle_empty', 'w3_seam', 'w4_one_row'])
@pytest.mark.parametrize('use_lnl', [False, True], ids=['diff', 'lnl'])
def test_uneven_shards(gpu_device, cut, use_lnl):
    """Explicit cuts with an empty rank, a rank without ambiguous rows, a rank of one row: every rank takes part in every collective
    with zero contributions.  Per rank what the single engine is held to; across the ranks pi, theta, lnl, n_iter and the per-call
    integers are the same bits; exclude / choose / conf match the single-engine run."""
    raw, key, cuts, capable = _cuts(cut)
    tr = base_trace(raw, key)
    world = len(cuts) - 1
    for t, chunks in ((3, (8, 8)), (5, (5, 11))):               # t = 3 inside a chunk; t = 5 ends a chunk
        eps = L.eps_for_stop(tr, t, use_lnl)
        out = _sharded(raw, tr, cuts, chunks, eps, use_lnl, '%s stop %d' % (cut, t))
        can = [o['info0']['lnl_fused'] == 1 and o['info0']['fused'] == 1 and o['info0']['nb'] > 0 for o in out]
        if use_lnl:
            assert all(can) == capable, ('which ranks can carry the lnl', cut, can, [o['info0'] for o in out])
        scheme = L.DIFF if not use_lnl else (L.LAGGED if all(can) else L.DEDICATED)
        script = L.script_of(L.chunk_script(chunks, L.flags_for(chunks), t, True, scheme))
        ref = _single_reference(raw, key, eps, use_lnl, T_BASE, 7)
        assert ref['n_iter'] == t
        for r, o in enumerate(out):
            assert (o['n'], o['conv']) == (t, True), (cut, r, o['n'], o['conv'])
            assert o['calls'] == script, (cut, 'rank', r, scheme, o['calls'], script)
            assert o['info']['fallbacks'] == 0, (cut, r, o['info'])
            assert _bits(o) == _bits(out[0]), (cut, 'rank', r, 'holds other bits than rank 0')
            assert np.array_equal(o['exclude'], ref['exclude']) and np.array_equal(o['choose'], ref['choose']), (cut, r, 'exclude / choose')
            assert np.array_equal(o['exclude'], tr.exclude_counts(t)), (cut, r, 'exclude against the reference')
            assert _frac(o['conf'], ref['conf'], 1e-9, 1e-12) <= 1.0, (cut, r, 'conf')
        _say('%s %s stop %d: world %d, scheme %s, rows %s, nb %s; lnl %.3g par %.3g diff %.3g of their tolerances', cut, 'lnl' if use_lnl else 'diff', t,
             world, scheme, np.diff(cuts).tolist(), [o['info0']['nb'] for o in out], *[max(o['frac'][i] for o in out) for i in range(3)])


@pytest.mark.parametrize('use_lnl', [False, True], ids=['diff', 'lnl'])
def test_timeout_on_a_rank_beside_an_empty_rank(gpu_device, use_lnl):
    """world 2, rank 1 empty, rank 0's second EM pass times out: nobody commits it, rank 0 alone falls back, both redo the iteration"""
    raw, key, cuts, _ = _cuts('w2_rank1_empty')
    tr = base_trace(raw, key)
    eps = L.eps_for_stop(tr, 5, use_lnl)
    out = _sharded(raw, tr, cuts, (8, 8), eps, use_lnl, 'time-out beside an empty rank', timeout_rank=0)
    for r, o in enumerate(out):
        assert (o['n'], o['conv']) == (5, True), (r, o['n'], o['conv'])
        assert _bits(o) == _bits(out[0])
        assert np.array_equal(o['exclude'], tr.exclude_counts(5))
    assert out[0]['info']['fallbacks'] == 1 and out[0]['info']['fused'] == 0, out[0]['info']
    assert out[1]['info']['fallbacks'] == 0, out[1]['info']
    assert out[0]['calls'] == out[1]['calls']


@pytest.mark.parametrize('name,world', [('tiny_one_row', 2), ('tiny_one_row', 8), ('tiny_unique_only', 8), ('tiny_twins', 8), ('tiny_ties_lnl', 8)])
def test_golden_cases_on_shard_bounds(gpu_device, name, world):
    """Golden cases cut by shard_bounds itself (as cli.py does) where that leaves empty shards: against the golden n_iter,
    converged, pi, theta, lnl and column sums, as test_chunked_protocol_between_two_ranks asserts them.  At world 8 eight persistent
    kernels share the device: a genuine watchdog fall-back is handled by the protocol under test, so only the results are asserted."""
    from telescope_amd.distributed import ThreadGroup, shard_bounds
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case(name)
    raw = case_matrix(c).tocsr()
    o = Opts(c)
    use_lnl = bool(c['use_likelihood'])
    cuts = shard_bounds(raw.shape[0], world, indptr=raw.indptr)
    assert min(np.diff(cuts)) == 0, ('no empty shard', cuts)
    group = ThreadGroup(0, world)
    group.set_timeout(RENDEZVOUS_S)

    def rank_main(rank):
        comm = group.comm(rank)
        try:
            r0, r1 = cuts[rank], cuts[rank + 1]
            tl = TelescopeLikelihood(raw[r0:r1], o, device=0, comm=comm, engine_options={'row_offset': r0})
            _track(tl._eng)
            tl.em(use_likelihood=use_lnl)
            res = dict(n_iter=tl.n_iter, converged=tl.converged, lnl=tl.lnl, pi=tl.pi.copy(), theta=tl.theta.copy(), pi_init=tl.pi_init.copy(),
                       fallbacks=tl._eng.layout_info()['fallbacks'])
            if rank == 0:
                np.random.seed(int(c['seed']))
            res['choose'] = tl.reassign_colsums('choose', 0.9, False)
            res['exclude'] = tl.reassign_colsums('exclude', 0.9, False)
            res['conf'] = tl.reassign_colsums('conf', 0.9, False)
            return res
        finally:
            comm.close()
    try:
        out = _run_ranks(world, rank_main, group.barrier)
    finally:
        group.close()
    for r in out:
        assert r['n_iter'] == int(c['n_iter']) and r['converged'] == bool(c['converged'])
        assert abs(r['lnl'] - float(c['lnl'])) <= 1e-10 * abs(float(c['lnl']))
        assert np.allclose(r['pi'], c['pi'], rtol=1e-10, atol=0) and np.allclose(r['theta'], c['theta'], rtol=1e-10, atol=0)
        assert np.allclose(r['pi_init'], c['pi_init'], rtol=1e-12, atol=0)
        assert np.array_equal(r['exclude'], c['ra_exclude_0_colsum']) and np.array_equal(r['choose'], c['ra_choose_0_colsum'])
        assert np.allclose(r['conf'], c['ra_conf_0_colsum'], rtol=1e-9, atol=1e-12)
        assert np.array_equal(r['pi'], out[0]['pi']) and np.array_equal(r['theta'], out[0]['theta']) and r['lnl'] == out[0]['lnl']
    _say('%s at world %d: rows per rank %s, fall-backs per rank %s', name, world, np.diff(cuts).tolist(), [r['fallbacks'] for r in out])
    if world <= 4:
        assert all(r['fallbacks'] == 0 for r in out)


# ---- D. k_local_reduce by itself ---------------------------------------------------------------------------------------------------
def _reduce_inputs(kind, op, world, count, seed):
    rng = np.random.RandomState(seed)
    if kind == 'f64' and op == 'sum':
        # values over 30 decades with both signs: the sum depends on the order of the additions
        a = rng.standard_normal((world, count)) * 10.0 ** rng.uniform(-15, 15, (world, count))
        a[:, 0] = [1.0, 1e16, -1e16, 3.0, 1e-3, -7.0, 0.5, 2.0][:world]            # in rank order the 1.0 is absorbed; in reverse order it survives
        return a
    if kind == 'u64':
        a = rng.randint(0, 2 ** 63 - 1, (world, count)).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        a[:, 0] = np.uint64(2 ** 64 - 1)                           # wraps
        return a
    if kind == 'i64':
        a = rng.randint(-2 ** 62, 2 ** 62, (world, count)).astype(np.int64)
        a[:, 0] = -np.arange(1, world + 1, dtype=np.int64) * 2 ** 40   # all negative
        if count > 1:
            a[:, 1] = np.iinfo(np.int64).min
            a[world - 1, 1] = np.iinfo(np.int64).min + 1
        return a
    a = rng.standard_normal((world, count)) * 10.0 ** rng.uniform(-300, 300, (world, count))
    a[:, 0] = -0.0
    if count > 1:
        a[:, 1] = 0.0
    if count > 2:
        a[:, 2] = -0.0
        a[world // 2, 2] = 0.0                                       # mixed zeros: the maximum is a zero of either sign
    if count > 3:
        a[:, 3] = -np.arange(1, world + 1) * 1e-310                  # negative subnormals
    return a


def _rank_order(a, kind, op):
    """the reduction in rank order, as k_local_reduce documents it"""
    v = a[0].copy()
    with np.errstate(over='ignore'):
        for q in range(1, a.shape[0]):
            v = v + a[q] if op == 'sum' else np.maximum(v, a[q])
    return v


@pytest.mark.parametrize('world', [3, 8])
def test_local_reduce(gpu_device, world):
    """k_local_reduce through LibComm.allreduce: all four dtype / op pairs, counts 1, 255, 256, 257 and 30 002.  f64 sums whose value
    depends on the order come out as the rank-order sum bit for bit (and a reversed order gives other bits: asserted on the
    inputs), u64 sums wrap, i64 max over negative values, f64 max over -0.0 and +0.0 (all -0.0 stays -0.0; of mixed zeros either
    zero is a maximum, numpy's comparison takes them as equal)."""
    from telescope_amd._lib import LocalGroup
    group = LocalGroup(0, world)
    group.set_timeout(RENDEZVOUS_S)
    cases = [(kind, op, count) for kind, op in (('f64', 'sum'), ('u64', 'sum'), ('f64', 'max'), ('i64', 'max')) for count in (1, 255, 256, 257, 30002)]
    inputs = {c: _reduce_inputs(c[0], c[1], world, c[2], 11 + i) for i, c in enumerate(cases)}

    def rank_main(rank):
        comm = group.comm(rank)
        try:
            return {c: comm.allreduce(inputs[c][rank], c[0], c[1]) for c in cases}
        finally:
            comm.close()
    try:
        out = _run_ranks(world, rank_main)
    finally:
        group.close()
    order_matters = 0
    for c in cases:
        kind, op, count = c
        want = _rank_order(inputs[c], kind, op)
        for r in range(world):
            got = out[r][c]
            assert got.dtype == want.dtype and got.shape == want.shape
            if kind == 'f64' and op == 'max':
                assert np.array_equal(got, want), (c, 'rank', r)
                assert np.signbit(got[0]) and (count < 2 or not np.signbit(got[1])), (c, 'the sign of an all -0.0 / all +0.0 maximum')
            else:
                assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (c, 'rank', r, np.flatnonzero(got != want)[:5])
        if kind == 'f64' and op == 'sum':
            rev = _rank_order(inputs[c][::-1], kind, op)
            order_matters += int(np.count_nonzero(rev.view(np.uint64) != want.view(np.uint64)))
            assert rev[0] != want[0], 'element 0 is built to depend on the order'
    assert order_matters > 0
    _say('local reduce, world %d: %d cases exact; %d f64 sums would differ in reverse rank order', world, len(cases), order_matters)


def test_zz_largest_errors():
    """the file's largest errors as fractions of their tolerances (printed for profiles/r24_em_loop.txt)"""
    _say('largest errors of the file: lnl %.3g, parameters %.3g, diff_est %.3g of their tolerances (1e-9, 1e-9, rtol 1e-7 + 1e-15)',
         _worst['lnl'], _worst['par'], _worst['diff'])
    assert max(_worst.values()) <= 1.0
