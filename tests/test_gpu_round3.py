"""Round-3 GPU tests (all through the C ABI, `-m gpu`):

* the SHIPPED chunked protocol (`tsem_em_chunk`: device-side stop flag, error slot K, pi_init capture, all-rank
  recovery, the 2-double lnl reduce) between TWO participants on one GPU through the library's in-process transport;
* the streaming report kernel against the generic row pass and the goldens;
* full-size oracle parity for BASELINE configs 2 and 3, a run that converges below max_iter on >= 1M rows;
* the order-deterministic final iteration.
"""
import os
import threading

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts, case_matrix, load_case

pytestmark = pytest.mark.gpu


def _run_ranks(world, fn):
    """fn(rank) on `world` host threads; re-raises the first failure."""
    out, errs = [None] * world, []

    def work(r):
        try:
            out[r] = fn(r)
        except BaseException as e:   # noqa: BLE001
            errs.append((r, e))
    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    [t.start() for t in ts]
    [t.join(900) for t in ts]
    assert not any(t.is_alive() for t in ts), 'a rank hangs'
    if errs:
        raise errs[0][1]
    return out


# ---------------------------------------------------------------------------------------------------
# tsem_em_chunk between two participants (VERDICT r2 #2 / missing #3)
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,fail_rank,fmt', [
    ('mid_zipf_20k', None, 0), ('bundled', None, 0), ('bundled_lnl', None, 0), ('tiny_ties_lnl', None, 0),
    ('tiny_twins', None, 0), ('mid_zipf_20k', None, 1),
    ('mid_zipf_20k', 1, 0), ('bundled_lnl', 0, 0), ('bundled_lnl', 1, 0),
    ('mid_zipf_20k', None, 'split'), ('bundled_lnl', None, 'split'), ('bundled_lnl', 1, 'split')])   # round 4: the split layout (two passes per iteration)
def test_chunked_protocol_between_two_ranks(gpu_device, name, fail_rank, fmt):
    """Two engines (rows split by nnz) as two threads with the in-process transport: the loop body is the shipped
    `tsem_em_chunk` — k_em_fused, k_colreduce, all-reduce of K+2 doubles, k_update, (lnl pass, all-reduce of 2
    doubles, k_lnl_check) per iteration, the device-side stop flag, one host synchronisation per chunk of EM_CHUNK.  Both
    ranks must stop in the reference's iteration with bit-identical parameters.  `fail_rank`: that rank's fused EM
    pass (and, with use_likelihood, its lnl pass) behaves like a hand-off time-out (fused_dbg bits 5 / 6): nobody
    commits, the failing rank alone rebuilds for the two-pass kernels, every rank redoes the iteration."""
    from telescope_amd.distributed import ThreadGroup, shard_bounds
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case(name)
    raw = case_matrix(c).tocsr()
    o = Opts(c)
    use_lnl = bool(c['use_likelihood'])
    group = ThreadGroup(0, 2)
    cuts = shard_bounds(raw.shape[0], 2, indptr=raw.indptr)

    def rank_main(rank):
        comm = group.comm(rank)
        r0, r1 = cuts[rank], cuts[rank + 1]
        opts = {'row_offset': r0, 'value_format': fmt} if fmt != 'split' else {'row_offset': r0, 'split': 1, 'parts': 5}
        if fail_rank == rank:
            opts['fused_dbg'] = 32 | (64 if use_lnl else 0)
        tl = TelescopeLikelihood(raw[r0:r1], o, device=0, comm=comm, engine_options=opts)
        assert tl._eng.layout_info()['fused'] == 1
        tl.em(use_likelihood=use_lnl)
        res = dict(n_iter=tl.n_iter, converged=tl.converged, lnl=tl.lnl, pi=tl.pi.copy(), theta=tl.theta.copy(),
                   pi_init=tl.pi_init.copy(), fallbacks=tl._eng.layout_info()['fallbacks'],
                   fused=tl._eng.layout_info()['fused'])
        if rank == 0:
            np.random.seed(int(c['seed']))
        res['choose'] = tl.reassign_colsums('choose', 0.9, False)
        res['exclude'] = tl.reassign_colsums('exclude', 0.9, False)
        res['conf'] = tl.reassign_colsums('conf', 0.9, False)
        comm.close()
        return res
    try:
        a, b = _run_ranks(2, rank_main)
    finally:
        group.close()
    for r in (a, b):
        assert r['n_iter'] == int(c['n_iter']) and r['converged'] == bool(c['converged'])
        assert abs(r['lnl'] - float(c['lnl'])) <= 1e-10 * abs(float(c['lnl']))
        assert np.allclose(r['pi'], c['pi'], rtol=1e-10, atol=0) and np.allclose(r['theta'], c['theta'], rtol=1e-10, atol=0)
        assert np.allclose(r['pi_init'], c['pi_init'], rtol=1e-12, atol=0)
        assert np.array_equal(r['exclude'], c['ra_exclude_0_colsum']) and np.array_equal(r['choose'], c['ra_choose_0_colsum'])
        assert np.allclose(r['conf'], c['ra_conf_0_colsum'], rtol=1e-9, atol=1e-12)
    assert np.array_equal(a['pi'], b['pi']) and np.array_equal(a['theta'], b['theta']) and a['lnl'] == b['lnl']
    if fail_rank is None:
        assert a['fallbacks'] == b['fallbacks'] == 0
    else:   # only the failing rank switched kernels
        got = (a, b)[fail_rank], (a, b)[1 - fail_rank]
        assert got[0]['fallbacks'] >= 1 and got[0]['fused'] == 0
        assert got[1]['fallbacks'] == 0 and got[1]['fused'] == 1


def test_second_run_compares_with_the_previous_lnl(gpu_device):
    """model.py:786: under use_likelihood the first iteration of a SECOND em() call is compared with self.lnl as the
    first call left it, not with inf: a converged model stops after one more iteration."""
    from telescope_amd.likelihood import TelescopeLikelihood
    from oracle.telescope_oracle import OracleModel
    c = load_case('bundled_lnl')
    raw = case_matrix(c)
    o = Opts(c)
    tl = TelescopeLikelihood(raw, o, device=0)
    tl.em(use_likelihood=True)
    n1 = tl.n_iter
    tl.em(use_likelihood=True)
    om = OracleModel(raw, o.pi_prior, o.theta_prior)
    om.em(o.em_epsilon, o.max_iter, True)
    assert n1 == om.n_iter == int(c['n_iter'])
    om.em(o.em_epsilon, o.max_iter, True)
    assert tl.n_iter == om.n_iter and tl.n_iter < n1
    assert abs(tl.lnl - om.lnl) <= 1e-10 * abs(om.lnl)
    ks = tl._eng.kernel_stats()       # em() switches the per-pass events off and must switch them back on
    tl._eng.em_steps(2)
    assert tl._eng.kernel_stats()['em_launches'] >= ks['em_launches'] + 1


# ---------------------------------------------------------------------------------------------------
# full-size oracle parity for BASELINE configs 2 and 3, short rows, a run that CONVERGES on >= 1M rows
# ---------------------------------------------------------------------------------------------------
RTOL = 1e-9


def _synthetic_tl(rows, cols, d, dist, seed=42, uniq=0.0, options=(), opts=None):
    from telescope_amd import _lib, synthetic
    from telescope_amd.likelihood import TelescopeLikelihood
    eng = _lib.Engine(0)
    for k, v in options:
        eng.set_option(k, v)
    eng.generate(0, rows, cols, synthetic.poisson_cdf_u32(d), seed, synthetic.DIST_CODE[dist], uniq)
    return TelescopeLikelihood.from_engine(eng, opts or Opts(max_iter=5, em_epsilon=0.0))


@pytest.mark.parametrize('rows,cols,d,fmt', [
    (1_000_000, 30_000, 20, 0),      # BASELINE config 2
    (1_000_000, 30_000, 20, 1),
    (10_000_000, 30_000, 40, 0),     # BASELINE config 3 (the precision sweep is bench.py's; this is its fp64 leg against the oracle)
    (10_000_000, 30_000, 40, 1),
    (1_000_000, 30_000, 18, 0),      # what real Telescope data looks like: the bundled matrix has 18.5 entries per row
    (2_000_000, 30_000, 10, 0),
])
def test_full_size_configs_against_the_c_oracle(gpu_device, rows, cols, d, fmt):
    """pi, theta, pi_init and lnl to 1e-9 against oracle/em_fused.c over the SAME matrix, the per-locus `exclude`
    counts bit for bit (same shape as the config-4 test of round 2)."""
    from oracle import em_fused as oc
    from telescope_amd._lib import Z_PREV
    iters = 5
    tl = _synthetic_tl(rows, cols, d, 'zipf', uniq=0.05, options=(('value_format', fmt),), opts=Opts(max_iter=iters, em_epsilon=0.0))
    tl.em()
    ip, ix, rw = tl._eng.export_csr()
    ref = oc.em_fused_arrays(ip, ix, rw, cols, 0, 200000, 0.0, iters)
    assert ref['n_iter'] == tl.n_iter == iters
    assert abs(tl.lnl - ref['lnl']) <= RTOL * abs(ref['lnl'])
    assert np.allclose(tl.pi, ref['pi'], rtol=RTOL, atol=0) and np.allclose(tl.theta, ref['theta'], rtol=RTOL, atol=0)
    assert np.allclose(tl.pi_init, ref['pi_init'], rtol=RTOL, atol=0)
    pp, tp = tl._eng.get_params(Z_PREV)
    want = oc.exclude_counts(ip, ix, rw, cols, pp, tp, max_score=tl.max_score)
    assert np.array_equal(tl.reassign_colsums('exclude'), want)
    assert np.array_equal(tl.reassign_colsums('exclude'), tl._eng.reassign('exclude', 0.9, Z_PREV)[0].astype(np.int64))   # both report kernels
    # the other two sums output_report takes from a z (model.py:432-457), final AND initial z, against oracle_report_sums: the
    # integer counts bit for bit, conf / average to summation order (1e-9: up to 1e6 terms per locus)
    for initial, prm in ((False, (pp, tp)), (True, (tl.pi, tl.theta))):
        conf, excl, avg = oc.report_sums(ip, ix, rw, cols, prm[0], prm[1], 0.9, initial, max_score=tl.max_score)
        assert np.array_equal(tl.reassign_colsums('exclude', initial=initial), excl)
        assert np.allclose(tl.reassign_colsums('conf', 0.9, initial=initial), conf, rtol=RTOL, atol=1e-9)
        assert np.allclose(tl.reassign_colsums('average', initial=initial), avg, rtol=RTOL, atol=1e-9)
        assert abs(avg.sum() - (rows - 0)) <= 1e-6 * rows            # every row with a pattern hands out exactly one unit


@pytest.mark.parametrize('rows,d,eps', [(1_000_000, 20, 1e-5), (2_000_000, 40, 2e-6)])
def test_device_side_convergence_below_max_iter_on_large_matrices(gpu_device, rows, d, eps):
    """model.py:792: `diff_est < epsilon` is decided ON THE DEVICE (k_update raises the stop flag mid-chunk).  On a
    >= 1M-row matrix the run must stop in the oracle's iteration — well below max_iter, so the count is the
    convergence test's, not the cap's — with the oracle's diff_est trace."""
    from oracle import em_fused as oc
    tl = _synthetic_tl(rows, 30_000, d, 'zipf', uniq=0.05, opts=Opts(max_iter=1000, em_epsilon=eps))
    tl.em()
    ip, ix, rw = tl._eng.export_csr()
    ref = oc.em_fused_arrays(ip, ix, rw, 30_000, 0, 200000, eps, 1000)
    assert ref['converged'] and tl.converged
    assert 8 < ref['n_iter'] < 1000 and tl.n_iter == ref['n_iter']
    assert abs(tl.lnl - ref['lnl']) <= RTOL * abs(ref['lnl'])
    assert np.allclose(tl.pi, ref['pi'], rtol=RTOL, atol=0)


@pytest.mark.parametrize('block_rows,fmt,parts', [(64, 0, 0), (128, 1, 0), (640, 0, 0), (1152, 1, 0), (0, 0, 4), (200, 0, 0)])
def test_short_row_geometry_with_any_block_size(gpu_device, block_rows, fmt, parts):
    """Geometry 3 of the fused kernel (rows so short that 768 of them cannot fill the register tile: the exchange wave
    keeps its own partial sums in registers from the publish to the combine and zeroes the 2-deep y ring at the
    publish) against the oracle — with forced block sizes far below what its three exchange waves cover: lanes clamped
    to the last row pair must neither zero nor publish it (a race found by test_random_shapes_against_oracle[3])."""
    from oracle.telescope_oracle import OracleModel
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    rng = np.random.RandomState(77)
    n, k = 30000, 16000
    lens = rng.randint(2, 7, n)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    data = rng.randint(139, 213, indptr[-1]).astype(np.uint16)
    raw = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    o = Opts(max_iter=4, em_epsilon=0.0)
    eng = _lib.Engine(0)
    eng.set_option('value_format', fmt)
    if block_rows:
        eng.set_option('block_rows', block_rows)
    if parts:
        eng.set_option('parts', parts)
    eng.load_scores(raw.indptr, raw.indices, raw.data, k, score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, o)
    tl._raw = raw
    tl.em()
    info = eng.layout_info()
    assert info['fused'] == 1 and info['geometry'] == 3, info
    om = OracleModel(raw, o.pi_prior, o.theta_prior)
    om.em(0.0, o.max_iter)
    assert abs(tl.lnl - om.lnl) <= RTOL * abs(om.lnl), info
    assert np.allclose(tl.pi, om.pi, rtol=RTOL, atol=1e-300) and np.allclose(tl.theta, om.theta, rtol=RTOL, atol=1e-300), info
    assert np.array_equal(tl.reassign_colsums('exclude'), np.asarray(om.reassign('exclude').sum(0)).ravel())


@pytest.mark.parametrize('split', [0, -1])
def test_report_pass_falls_back_beyond_65536_slots(gpu_device, split):
    """The streaming report kernel indexes LDS with 16-bit popularity ids; a matrix with more column slots than that
    (K = 70 000: ten column parts on the two-pass EM kernels, or — round 4 — the split layout of the fused kernel) must take
    the generic row pass — and agree with the oracle."""
    from oracle.telescope_oracle import OracleModel
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    rng = np.random.RandomState(5)
    n, k = 8000, 70000
    lens = np.where(rng.rand(n) < 0.1, 1, rng.randint(2, 30, n))
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    data = rng.randint(139, 213, indptr[-1]).astype(np.uint16)
    raw = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    o = Opts(max_iter=3, em_epsilon=0.0)
    eng = _lib.Engine(0)
    eng.set_option('split', split)
    eng.load_scores(raw.indptr, raw.indices, raw.data, k, score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, o)
    tl._raw = raw
    tl.em()
    info = eng.layout_info()
    assert info['fused'] == (0 if split == 0 else 1) and info['split'] == (0 if split == 0 else 1) and info['P'] * info['Kp'] > 65536, info
    om = OracleModel(raw, o.pi_prior, o.theta_prior)
    om.em(0.0, o.max_iter)
    assert abs(tl.lnl - om.lnl) <= RTOL * abs(om.lnl)
    np.random.seed(3); got = {m: tl.reassign_colsums(m, 0.9, init) for m, init in (('exclude', False), ('choose', True), ('average', True), ('conf', False))}
    np.random.seed(3)
    assert np.array_equal(got['exclude'], np.asarray(om.reassign('exclude').sum(0)).ravel())
    assert np.array_equal(got['choose'], np.asarray(om.reassign('choose', initial=True).sum(0)).ravel())
    assert np.allclose(got['average'], np.asarray(om.reassign('average', initial=True).sum(0)).ravel(), rtol=1e-12, atol=1e-12)
    assert np.allclose(got['conf'], np.asarray(om.reassign('conf', 0.9).sum(0)).ravel(), rtol=1e-12, atol=1e-12)


# ---------------------------------------------------------------------------------------------------
# option "reproducible": order-independent column sums
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,d,fmt', [(300_000, 24, 0), (5_000_000, 40, 0), (2_000_000, 10, 1)])
def test_reproducible_mode_is_bitwise_reproducible(gpu_device, rows, d, fmt):
    """With `reproducible` = 1 every contribution to a column sum is split into pieces whose sums are exact in fp64, so the
    unordered LDS atomics of the fused pass add up to the same bits in every run: pi, theta, lnl and the iteration count
    of two independent runs are IDENTICAL — and agree with the C oracle like the default
    mode does.  The default mode is checked to be only tolerance-equal on the same matrix (if it ever becomes bitwise
    equal by itself this assertion can go)."""
    from oracle import em_fused as oc
    runs = []
    for rep in range(2):
        tl = _synthetic_tl(rows, 30_000, d, 'zipf', uniq=0.05, options=(('value_format', fmt), ('reproducible', 1)),
                           opts=Opts(max_iter=200, em_epsilon=1e-4))
        tl.em()
        info = tl._eng.layout_info()
        assert info['reproducible'] == 1 and info['fused'] == 1
        runs.append((tl.n_iter, tl.pi.copy(), tl.theta.copy(), tl.lnl, tl.pi_init.copy(), info['bin_repeats']))
        if rep == 0:
            ip, ix, rw = tl._eng.export_csr()
            ref = oc.em_fused_arrays(ip, ix, rw, 30_000, 0, 200000, 1e-4, 200)
        del tl
    a, b = runs
    assert a[0] == b[0] == ref['n_iter'] and 3 < a[0] < 200
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and np.array_equal(a[4], b[4])
    assert a[5] == b[5] and a[5] <= 4 + a[0] // 2, a[5]          # passes repeated because a column's grid had to move
    print('reproducible: %d iterations, %d repeated passes' % (a[0], a[5]))
    assert abs(a[3] - ref['lnl']) <= RTOL * abs(ref['lnl'])
    assert np.allclose(a[1], ref['pi'], rtol=RTOL, atol=0) and np.allclose(a[2], ref['theta'], rtol=RTOL, atol=0)


def test_reproducible_mode_on_goldens(gpu_device):
    """The same option on the reference's golden cases (tiny matrices, exact twins): same iteration counts and outputs as
    the default mode's tests demand.  A case the mode cannot take (a 65 535-wide score range does not fit the LDS table)
    is an ERROR at set-up, not a silent switch to the order-dependent path."""
    from telescope_amd.likelihood import TelescopeLikelihood
    from telescope_amd._lib import EngineError
    ran = []
    for name in ('bundled', 'tiny_twins', 'tiny_ties', 'tiny_wide_range', 'mid_zipf_20k', 'bundled_lnl'):
        c = load_case(name)
        raw = case_matrix(c)
        res = []
        for rep in range(2):
            try:
                tl = TelescopeLikelihood(raw, Opts(c), device=0, engine_options={'reproducible': 1})
            except EngineError as e:
                assert 'reproducible mode needs' in str(e), name
                break
            assert tl._eng.layout_info()['fused'] == 1 and tl._eng.layout_info()['reproducible'] == 1
            tl.em(use_likelihood=bool(c['use_likelihood']))
            res.append((tl.n_iter, tl.pi.copy(), tl.lnl, tl.reassign_colsums('exclude')))
        if not res:
            continue
        ran.append(name)
        assert res[0][0] == res[1][0] == int(c['n_iter']), name
        assert np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2], name
        assert np.allclose(res[0][1], c['pi'], rtol=1e-10, atol=0) and abs(res[0][2] - float(c['lnl'])) <= 1e-10 * abs(float(c['lnl'])), name
        assert np.array_equal(res[0][3], c['ra_exclude_0_colsum']), name
    print('reproducible goldens:', ran)
    assert len(ran) >= 4, ran

# (round 3's test_reproducible_mode_has_no_order_dependent_fallback expected the run to END with an error after a time-out; since round 4
#  the pass is redone on the fused kernel: tests/test_gpu_round4.py::test_reproducible_mode_redoes_a_timed_out_pass_on_the_fused_kernel)


def test_reproducible_report_sums_are_bitwise_reproducible(gpu_device):
    """The float-valued report columns (`conf`, `average` of TE_counts.tsv, model.py:455-458) under `reproducible`: every
    value is cut into two pieces whose sums are exact (exact_split01), in the streaming report kernel, in the generic row
    pass and in the per-barcode pass alike — two independent contexts give the same bits; against the default mode the
    sums agree to rounding."""
    from telescope_amd._lib import Z_PREV, Z_INITIAL
    rows = 2_000_000
    groups = [np.arange(0, rows, 7), np.arange(3, rows, 11), np.array([5, 5, 9])]
    got = {}
    for mode in ('default', 'a', 'b'):
        options = () if mode == 'default' else (('reproducible', 1),)
        tl = _synthetic_tl(rows, 30_000, 24, 'zipf', uniq=0.05, options=options, opts=Opts(max_iter=6, em_epsilon=0.0))
        tl.em()
        res = {}
        for kern in (1, 0):
            tl._eng.set_option('report_kernel', kern)
            for which in (Z_PREV, Z_INITIAL):
                sums, r, c = tl._eng.report_colsums(which, 0.9)
                res[(kern, which)] = (sums['conf'].copy(), sums['average'].copy(), sums['exclude'].copy(), r.copy(), c.copy())
        tl._eng.set_option('report_kernel', 1)
        res['conf_single'] = tl._eng.reassign('conf', 0.9, Z_PREV)[0].copy()
        res['avg_single'] = tl._eng.reassign('average', 0.9, Z_PREV)[0].copy()
        res['groups'] = tl.reassign_group_sums('conf', groups, 0.9).copy()
        got[mode] = res
        del tl
    a, b, d = got['a'], got['b'], got['default']
    for key in a:
        if isinstance(a[key], tuple):
            for x, y, z in zip(a[key], b[key], d[key]):
                assert np.array_equal(x, y), key
                assert np.allclose(x, z, rtol=1e-11, atol=1e-9), key
        else:
            assert np.array_equal(a[key], b[key]), key
            assert np.allclose(a[key], d[key], rtol=1e-11, atol=1e-9), key
    # the two kernels compute a row's posteriors with different (fixed) reduction trees: equal to rounding, not bit for bit
    assert np.allclose(a[(1, Z_PREV)][0], a[(0, Z_PREV)][0], rtol=1e-11, atol=1e-9)
    assert np.array_equal(a[(1, Z_PREV)][2], a[(0, Z_PREV)][2])
    assert float(a[(1, Z_PREV)][0].sum()) > 1e5                  # (not vacuous)


def test_reproducible_mode_between_two_ranks(gpu_device):
    """Row shards on two participants (in-process transport, the shipped chunk loop) with `reproducible`: each rank's sums
    are exact, the all-reduce adds them in rank order — two executions give the same bits on both ranks, and the golden
    result."""
    from telescope_amd.distributed import ThreadGroup, shard_bounds
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case('mid_zipf_20k')
    raw = case_matrix(c).tocsr()
    o = Opts(c)
    cuts = shard_bounds(raw.shape[0], 2, indptr=raw.indptr)
    runs = []
    for execution in range(2):
        group = ThreadGroup(0, 2)

        def rank_main(rank):
            comm = group.comm(rank)
            r0, r1 = cuts[rank], cuts[rank + 1]
            tl = TelescopeLikelihood(raw[r0:r1], o, device=0, comm=comm,
                                     engine_options={'row_offset': r0, 'reproducible': 1})
            assert tl._eng.layout_info()['fused'] == 1 and tl._eng.layout_info()['reproducible'] == 1
            tl.em()
            res = (tl.n_iter, tl.lnl, tl.pi.copy(), tl.theta.copy(), tl.reassign_colsums('conf', 0.9, False).copy())
            comm.close()
            return res
        try:
            runs.append(_run_ranks(2, rank_main))
        finally:
            group.close()
    (a0, a1), (b0, b1) = runs
    for x in (a1, b0, b1):
        assert x[0] == a0[0] == int(c['n_iter']) and x[1] == a0[1]
        assert np.array_equal(x[2], a0[2]) and np.array_equal(x[3], a0[3]) and np.array_equal(x[4], a0[4])
    assert np.allclose(a0[2], c['pi'], rtol=1e-10, atol=0) and abs(a0[1] - float(c['lnl'])) <= 1e-10 * abs(float(c['lnl']))
    assert np.allclose(a0[4], c['ra_conf_0_colsum'], rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize('seed', range(16))
def test_reproducible_mode_on_random_shapes(gpu_device, seed):
    """The shapes of test_random_shapes_against_oracle (1..5 column parts, one block or many, rows of 1..120 entries,
    0..60 % single-entry rows, forced block sizes, priors on and off — with both priors 0 columns die and their grids must
    follow them down) under `reproducible`: two contexts agree bit for bit, and with the oracle to the usual tolerance.  A
    shape the mode cannot take must be refused at set-up."""
    import scipy.sparse as sp
    from oracle.telescope_oracle import OracleModel
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    rng = np.random.RandomState(7000 + seed)
    k = int(rng.choice([3, 17, 200, 5000, 9000, 16000, 24000, 33000]))
    n = int(rng.choice([7, 300, 2500, 12000, 40000]))
    max_len = int(min(k, rng.choice([2, 5, 30, 120])))
    uniq = float(rng.choice([0.0, 0.1, 0.6]))
    lens = np.where(rng.rand(n) < uniq, 1, rng.randint(1, max_len + 1, n))
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    lo, hi = [(139, 212), (1, 5), (100, 1500), (60000, 65535)][int(rng.randint(4))]
    data = rng.randint(lo, hi + 1, indptr[-1]).astype(np.uint16)
    raw = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    options = [('reproducible', 1)]
    if rng.rand() < 0.3:
        options.append(('block_rows', int(rng.choice([64, 128, 256]))))
    o = Opts(max_iter=int(rng.randint(2, 12)), em_epsilon=0.0)
    o.pi_prior, o.theta_prior = [(0, 200000), (0, 0), (5, 1000)][int(rng.randint(3))]
    res = []
    for rep in range(2):
        eng = _lib.Engine(0)
        for key, v in options:
            eng.set_option(key, v)
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), k, score_lut(int(raw.data.max())))
        try:
            tl = TelescopeLikelihood.from_engine(eng, o)
        except _lib.EngineError as e:
            assert 'reproducible mode needs' in str(e)
            assert hi > 2047 or eng.layout_info()['fused'] == 0, (seed, n, k, hi)   # the documented limits, nothing else
            return
        tl._raw = raw
        tl.em()
        res.append((tl.lnl, tl.pi.copy(), tl.theta.copy(), tl.reassign_colsums('conf').copy(), eng.layout_info()))
    a, b = res
    ctx = (seed, n, k, max_len, uniq, (lo, hi), options, a[4])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), ctx
    om = OracleModel(raw, o.pi_prior, o.theta_prior)
    om.em(0.0, o.max_iter)
    assert abs(a[0] - om.lnl) <= RTOL * max(abs(om.lnl), 1e-300), ctx
    assert np.allclose(a[1], om.pi, rtol=RTOL, atol=1e-300) and np.allclose(a[2], om.theta, rtol=RTOL, atol=1e-300), ctx
    assert np.allclose(a[3], np.asarray(om.reassign('conf').sum(0)).ravel(), rtol=1e-9, atol=1e-12), ctx


def test_reproducible_mode_reports_rows_it_cannot_vouch_for(gpu_device):
    """A row of more than 256 entries can end in three row-sum atomics (a run across three wavefronts), whose order is
    the hardware's: tsem_layout_info[21] says 2 instead of 1 then (include/telescope_em.h); the results stay within the
    usual tolerance of the oracle."""
    import scipy.sparse as sp
    from oracle.telescope_oracle import OracleModel
    from telescope_amd.likelihood import TelescopeLikelihood
    rng = np.random.RandomState(5)
    n, k = 3000, 6000
    lens = rng.randint(2, 20, n)
    lens[17] = 700
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    raw = sp.csr_matrix((rng.randint(100, 300, indptr[-1]).astype(np.uint16), indices, indptr), shape=(n, k))
    o = Opts(max_iter=4, em_epsilon=0.0)
    tl = TelescopeLikelihood(raw, o, device=0, engine_options={'reproducible': 1})
    assert tl._eng.layout_info()['reproducible'] == 2
    tl.em()
    om = OracleModel(raw, o.pi_prior, o.theta_prior)
    om.em(0.0, o.max_iter)
    assert abs(tl.lnl - om.lnl) <= RTOL * abs(om.lnl) and np.allclose(tl.pi, om.pi, rtol=RTOL, atol=0)
    lens[17] = 200
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    raw = sp.csr_matrix((rng.randint(100, 300, indptr[-1]).astype(np.uint16), indices, indptr), shape=(n, k))
    assert TelescopeLikelihood(raw, o, device=0, engine_options={'reproducible': 1})._eng.layout_info()['reproducible'] == 1


_BENCH_COMMON = ['--rows', '3000000', '--steps', '6', '--warmup', '2', '--no-cpu-baseline', '--no-alt-layout', '--no-precision-sweep',
                 '--no-reproducible-leg', '--uniq-frac', '0.05', '--full']
_BENCH_LINES = {}


def _bench_line(key, prefix, extra):
    import json
    import subprocess
    if key not in _BENCH_LINES:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        r = subprocess.run(prefix + [os.path.join(root, 'bench.py')] + extra + _BENCH_COMMON, cwd=root, capture_output=True, text=True,
                           timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        _BENCH_LINES[key] = json.loads(r.stdout.strip().splitlines()[-1])
    return _BENCH_LINES[key]


@pytest.mark.parametrize('launcher', ['self', 'torchrun'])
def test_bench_two_ranks_dry_run_on_one_gpu(gpu_device, launcher):
    """`python bench.py --gpus 2 --one-device` (bench.py starts the ranks) and the driver's form `python -m
    torch.distributed.run --nproc-per-node 2 ... bench.py --gpus 2 --one-device`: two rank processes that share GPU 0 (gloo, the
    reduce buffer staged through the host — RCCL refuses two ranks on one device): row shards generated from the global row index,
    the set-up collectives, one all-reduce per iteration, MAX of the elapsed times, rank 0's result line.  Its `check` block (the
    parameters after warm-up + steps folded to three numbers) must equal the single-process run's."""
    import socket
    import sys as _sys
    one = _bench_line('one', [_sys.executable], ['--gpus', '1'])
    if launcher == 'self':
        two = _bench_line('self', [_sys.executable], ['--gpus', '2', '--one-device'])
    else:
        sk = socket.socket(); sk.bind(('127.0.0.1', 0)); port = sk.getsockname()[1]; sk.close()
        two = _bench_line('torchrun', [_sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                                       '--master-addr', '127.0.0.1', '--master-port', str(port)], ['--gpus', '2', '--one-device'])
    assert two['n_gpus'] == 2 and one['n_gpus'] == 1 and two['config']['nnz'] == one['config']['nnz']
    assert 'DRY RUN' in two['config']['transport']
    assert ('self' in two['config']['launcher']) == (launcher == 'self')
    assert two['check']['iterations'] == one['check']['iterations'] == 8
    for key in ('pi_sum', 'pi_weighted', 'theta_weighted'):
        assert abs(two['check'][key] - one['check'][key]) <= 1e-11 * abs(one['check'][key]), key
    assert two['value'] > 0 and two['ms_per_step'] > 0
    # round 5: the line validates and diagnoses itself — its own N = 1 reference (whole problem on rank 0's GPU, same process) agrees
    # with the two-rank parameters; the phases of an iteration were timed on rank 0 (here: the host-driven fall-back transport)
    assert two['check']['matches_n1'] is True and two['n1_reference']['check']['iterations'] == 8, two['check']
    assert two['speedup_vs_n1'] is not None and two['speedup_vs_n1'] > 0
    for line in (one, two):
        ph = line['phase_us']
        assert ph and ph['iterations'] >= 4 and ph['pass'] > 0 and ph['update'] > 0, ph
    assert two['phase_us']['allreduce'] > 0 and one['phase_us']['allreduce'] < 50.0
    assert one['check']['matches_n1'] is None                      # (not the default workload: no embedded reference)


def test_reproducible_one_pass_and_two_pass_forms(gpu_device):
    """`reproducible` = 1 takes the ONE-pass form (three tables per part in LDS: both pieces of every contribution in one
    launch) where it fits — K = 15k with teams of 4 — and = 2 forces the two-pass form; each is bitwise reproducible, both agree
    with the C oracle like the default mode, and with long rows K = 30k takes the one-pass form with teams of 7-8."""
    from oracle import em_fused as oc
    res = {}
    for form in (1, 2):
        runs = []
        for rep in range(2):
            tl = _synthetic_tl(1_500_000, 15_000, 24, 'zipf', uniq=0.05, options=(('reproducible', form),),
                               opts=Opts(max_iter=12, em_epsilon=0.0))
            info = tl._eng.layout_info()
            assert info['exact_single'] == (1 if form == 1 else 0) and info['reproducible'] == 1
            tl.em()
            runs.append((tl.lnl, tl.pi.copy(), tl.theta.copy()))
            if form == 1 and rep == 0:
                ip, ix, rw = tl._eng.export_csr()
                ref = oc.em_fused_arrays(ip, ix, rw, 15_000, 0, 200000, 0.0, 12)
        assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][2], runs[1][2])
        res[form] = runs[0]
    for form in (1, 2):
        assert abs(res[form][0] - ref['lnl']) <= RTOL * abs(ref['lnl'])
        assert np.allclose(res[form][1], ref['pi'], rtol=RTOL, atol=0) and np.allclose(res[form][2], ref['theta'], rtol=RTOL, atol=0)
    tl = _synthetic_tl(300_000, 30_000, 100, 'zipf', uniq=0.05, options=(('reproducible', 1),), opts=Opts(max_iter=4, em_epsilon=0.0))
    info = tl._eng.layout_info()
    assert info['exact_single'] == 1 and info['P'] >= 7
    tl.em()
    ip, ix, rw = tl._eng.export_csr()
    ref = oc.em_fused_arrays(ip, ix, rw, 30_000, 0, 200000, 0.0, 4)
    assert abs(tl.lnl - ref['lnl']) <= RTOL * abs(ref['lnl']) and np.allclose(tl.pi, ref['pi'], rtol=RTOL, atol=0)


@pytest.mark.parametrize('cols,d,fmt', [(40_000, 20, 0), (50_000, 36, 0), (33_000, 12, 1), (61_000, 24, 0)])
def test_teams_of_5_to_8_with_768_row_slots(gpu_device, cols, d, fmt):
    """K in (30k, 61k] needs teams of 5-8; when their rows are too short to fill the register tiles with 384 row slots they now
    take the 768-slot geometry (two row pairs per exchange lane): against the C oracle, and against the 384-slot geometry."""
    from oracle import em_fused as oc
    tl = _synthetic_tl(400_000, cols, d, 'zipf', uniq=0.05, options=(('value_format', fmt),), opts=Opts(max_iter=5, em_epsilon=0.0))
    info = tl._eng.layout_info()
    assert info['fused'] == 1 and info['P'] >= 5 and info['geometry'] == 2 and info['R'] > 384, info
    tl.em()
    ip, ix, rw = tl._eng.export_csr()
    ref = oc.em_fused_arrays(ip, ix, rw, cols, 0, 200000, 0.0, 5)
    assert abs(tl.lnl - ref['lnl']) <= RTOL * abs(ref['lnl'])
    assert np.allclose(tl.pi, ref['pi'], rtol=RTOL, atol=0) and np.allclose(tl.theta, ref['theta'], rtol=RTOL, atol=0)
    t1 = _synthetic_tl(400_000, cols, d, 'zipf', uniq=0.05, options=(('value_format', fmt), ('geometry', 1)), opts=Opts(max_iter=5, em_epsilon=0.0))
    assert t1._eng.layout_info()['geometry'] == 1 and t1._eng.layout_info()['R'] <= 384
    t1.em()
    assert abs(t1.lnl - tl.lnl) <= 1e-11 * abs(tl.lnl) and np.allclose(t1.pi, tl.pi, rtol=1e-10, atol=0)
    assert np.array_equal(t1.reassign_colsums('exclude'), tl.reassign_colsums('exclude'))
