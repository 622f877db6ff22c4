"""Bootstrap replicates on the device (`TelescopeLikelihood.bootstrap`, tsem_bootstrap) against their definition: the oracle's fit of
the matrix in which every row appears as often as its multiplicity says, with the score scale of the whole matrix — iteration counts,
convergence and fragment counts equal, pi / theta / lnl at RTOL, integer counts equal and float counts at RTOL; every batch and
accumulator path; explicit multiplicities and their edge cases; twins; the pooled state left alone; `resume --bootstrap` end to end.

Cases (tests/_bootstrap_reference.py): C1-C4 with replicates 0..4 of seed 7; each reference is computed once per session.  Every
comparison first asserts of its own reference that no row is undecided (two best z, or a z and conf_prob, within 1e-9 relative) and
that no stop test lies within 1e-6 relative of epsilon, so exact comparison of integer counts and iteration counts is fair."""
import functools
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import Opts
import _bootstrap_reference as B
from _bootstrap_reference import RTOL

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = sorted(B.CASES)


def _tl(raw, pi_prior, theta_prior, device=0, **engine_options):
    from telescope_amd.likelihood import TelescopeLikelihood
    return TelescopeLikelihood(raw, Opts(pi_prior=pi_prior, theta_prior=theta_prior, em_epsilon=B.EPSILON, max_iter=B.MAX_ITER),
                               device=device, engine_options=engine_options or None)


@functools.lru_cache(maxsize=None)
def _case_tl(name):
    _, _, _, pp, tp = B.CASES[name]
    return _tl(B.case_matrix(name), pp, tp)


@functools.lru_cache(maxsize=None)
def _case_fits(name, method):
    return _case_tl(name).bootstrap(len(B.REPS), seed=B.SEED, method=method, thresh=B.CONF)


def _fair(ref):
    assert ref.undecided() == 0
    assert ref.stop_margin() > 1e-6, ref.stop_margin()


def _check_counts(fits, ref, method, label):
    for b, om in enumerate(ref.fits):
        want = ref.counts(b, method)
        if method in B.INT_METHODS:
            assert np.array_equal(fits.counts[b], want), (label, method, b, np.flatnonzero(fits.counts[b] != want)[:5])
        else:
            assert np.allclose(fits.counts[b], want, rtol=RTOL, atol=0), (label, method, b)


def test_the_cases_do_what_they_were_chosen_for():
    """C1: early finishers, max_iter with and without convergence; C3: all five at max_iter; C2, C4 short runs without NaN."""
    r1 = B.case_ref('C1')
    assert [(om.n_iter, bool(om.converged)) for om in r1.fits] == [(100, False), (76, True), (100, True), (100, False), (52, True)]
    assert all(om.n_iter == 100 and not om.converged for om in B.case_ref('C3').fits)
    assert all(10 <= om.n_iter <= 15 for om in B.case_ref('C2').fits)
    assert all(30 <= om.n_iter <= 46 and not np.isnan(om.pi).any() for om in B.case_ref('C4').fits)


@pytest.mark.parametrize('name', CASES)
def test_replicates_equal_the_oracle(gpu_device, name):
    ref = B.case_ref(name)
    _fair(ref)
    fits = _case_fits(name, 'exclude')
    assert fits.fitted.all()
    B.check_replicates(fits, ref, name)


@pytest.mark.parametrize('name', CASES)
def test_counts_of_every_method_equal_the_oracle(gpu_device, name):
    ref = B.case_ref(name)
    _fair(ref)
    for method in B.METHODS:
        fits = _case_fits(name, method)
        B.check_replicates(fits, ref, (name, method))
        _check_counts(fits, ref, method, name)


@pytest.mark.parametrize('name', ['C1', 'C3'])
def test_batch_and_accumulator_paths(gpu_device, name):
    """5 replicates over batches of 2 with a remainder, K above (C3) and below (C1) the hot columns, LDS and global accumulators,
    and the defaults: `info` reports what was used, results equal the oracle's every time."""
    ref = B.case_ref(name)
    _fair(ref)
    raw = B.case_matrix(name)
    _, _, k, pp, tp = B.CASES[name]
    ncols = int((np.bincount(raw.indices, minlength=k) > 0).sum())
    for opts, want in (({'boot_batch': 2, 'boot_hot_columns': 64}, {'batch': 2, 'hot_columns': min(64, ncols)}),
                       ({'boot_hot_columns': 0}, {'batch': 5, 'hot_columns': 0}),
                       ({}, {'batch': 5, 'hot_columns': min(4096 // 5, ncols)})):
        tl = _tl(raw, pp, tp, **opts)
        fits = tl.bootstrap(len(B.REPS), seed=B.SEED)
        assert fits.info == want, (name, opts, fits.info)
        B.check_replicates(fits, ref, (name, tuple(opts.items())))
        _check_counts(fits, ref, 'exclude', name)
    assert (name == 'C1') == (want['hot_columns'] == ncols)    # C1: every column is hot; C3: more columns than LDS slots


def test_eight_replicates_fill_a_batch_and_long_rows_take_several_strides(gpu_device):
    """Nine replicates = a full batch of 8 and one more; rows of up to 40 entries (more than the 8 lanes of a row, and than any row of
    C1-C4), a third of them on the first 16 columns (hot) at boot_hot_columns = 16."""
    rng = np.random.RandomState(40)
    n, k = 1200, 300
    lens = rng.randint(1, 41, n)
    lens[rng.rand(n) < 0.3] = 1
    idx = []
    for l in lens:
        hot = rng.choice(16, min(l // 3, 16), replace=False)
        rest = 16 + rng.choice(k - 16, l - len(hot), replace=False)
        idx.append(np.sort(np.concatenate([hot, rest])))
    indptr = np.concatenate([[0], np.cumsum(lens)])
    raw = sp.csr_matrix((rng.randint(100, 400, indptr[-1]).astype(np.uint16), np.concatenate(idx).astype(np.int32), indptr), shape=(n, k))
    mult = B.default_multiplicities(n, seed=5, reps=range(9))
    ref = B.BootRef(raw, mult, 0, 200000, max_iter=30)
    _fair(ref)
    from telescope_amd.likelihood import TelescopeLikelihood
    tl = TelescopeLikelihood(raw, Opts(max_iter=30), device=gpu_device, engine_options={'boot_hot_columns': 16})
    fits = tl.bootstrap(9, seed=5, method='average')
    assert fits.info == {'batch': 8, 'hot_columns': 16}
    B.check_replicates(fits, ref, 'long rows')
    _check_counts(fits, ref, 'average', 'long rows')


def test_device_multiplicities_equal_the_host_function(gpu_device):
    from telescope_amd.synthetic import bootstrap_multiplicities
    tl = _case_tl('C2')
    n = tl.N
    for rep in (0, 3):
        assert np.array_equal(tl._eng.bootstrap_mult(B.SEED, rep, 0, n), bootstrap_multiplicities(B.SEED, rep, np.arange(n)))
    assert np.array_equal(tl._eng.bootstrap_mult(2 ** 63 + 5, 1, 100, 777), bootstrap_multiplicities(2 ** 63 + 5, 1, np.arange(100, 777)))
    assert len(tl._eng.bootstrap_mult(1, 0, 5, 5)) == 0
    from telescope_amd._lib import EngineError
    with pytest.raises(EngineError):
        tl._eng.bootstrap_mult(1, 0, 0, n + 1)


def test_default_multiplicities_are_what_the_fit_uses(gpu_device):
    """Explicit multiplicities equal to the default draws give the default call's results (n_frags included)."""
    tl = _case_tl('C2')
    a = _case_fits('C2', 'exclude')
    b = tl.bootstrap(len(B.REPS), method='exclude', multiplicities=B.default_multiplicities(tl.N))
    assert np.array_equal(a.n_frags, b.n_frags) and np.array_equal(a.n_iter, b.n_iter) and np.array_equal(a.converged, b.converged)
    assert np.allclose(a.pi, b.pi, rtol=RTOL, atol=0) and np.allclose(a.lnl, b.lnl, rtol=RTOL, atol=0)
    assert np.array_equal(a.counts, b.counts)


def test_explicit_multiplicities(gpu_device):
    """All ones = the pooled fit; all zeros = not fitted; zero on every ambiguous row, and 255 on ten rows, as the oracle."""
    raw = B.case_matrix('C2')
    _, n, k, pp, tp = B.CASES['C2']
    rng = np.random.RandomState(3)
    mult = np.ones((4, n), np.uint8)
    mult[1] = 0
    mult[2, np.diff(raw.indptr) > 1] = 0
    mult[3, rng.choice(n, 10, replace=False)] = 255
    ref = B.BootRef(raw, mult, pp, tp)
    _fair(ref)
    tl = _case_tl('C2')
    fits = tl.bootstrap(4, method='exclude', multiplicities=mult)
    B.check_replicates(fits, ref, 'explicit')
    assert list(fits.fitted) == [True, False, True, True]
    for b in (0, 2, 3):
        assert np.array_equal(fits.counts[b], ref.counts(b, 'exclude')), b
    pooled = _tl(raw, pp, tp)
    pooled.em()
    assert fits.n_iter[0] == pooled.n_iter and bool(fits.converged[0]) == bool(pooled.converged)
    assert np.allclose(fits.pi[0], pooled.pi, rtol=RTOL, atol=0) and np.allclose(fits.theta[0], pooled.theta, rtol=RTOL, atol=0)
    assert np.isclose(fits.lnl[0], pooled.lnl, rtol=RTOL, atol=0)
    assert np.array_equal(fits.counts[0], pooled.reassign_colsums('exclude'))


def test_unique_rows_only_at_theta_prior_zero(gpu_device):
    """No ambiguous fragment and theta_prior = 0: theta = 0 / 0; pi and theta NaN, max_iter reached unconverged — what the oracle
    gives — and NaN counts and lnl."""
    rng = np.random.RandomState(5)
    n, k = 300, 20
    raw = sp.csr_matrix((rng.randint(100, 400, n).astype(np.uint16), (np.arange(n), rng.randint(0, k, n))), shape=(n, k))
    mult = B.default_multiplicities(n, reps=(0, 1))
    ref = B.BootRef(raw, mult, 0, 0)
    for om in ref.fits:
        assert np.isnan(om.pi).all() and np.isnan(om.theta).all() and om.n_iter == B.MAX_ITER and not om.converged and np.isnan(om.lnl)
    fits = _tl(raw, 0, 0).bootstrap(2, seed=B.SEED)
    B.check_replicates(fits, ref, 'unique only')
    assert np.isnan(fits.pi).all() and np.isnan(fits.theta).all() and np.isnan(fits.counts).all() and np.isnan(fits.lnl).all()
    assert list(fits.n_iter) == [B.MAX_ITER] * 2 and not fits.converged.any() and not fits.fitted.any()


def test_twins_tie_in_every_replicate(gpu_device):
    raw, _, _ = B.twin_tie_matrix()
    n = raw.shape[0]
    amb = np.diff(raw.indptr) > 1
    mult = B.default_multiplicities(n)
    ref = B.BootRef(raw, mult, 0, 200000)
    assert all(om.n_iter == 2 for om in ref.fits)
    tl = _tl(raw, 0, 200000)
    ex = tl.bootstrap(len(B.REPS), seed=B.SEED, method='exclude')
    av = tl.bootstrap(len(B.REPS), seed=B.SEED, method='average')
    B.check_replicates(ex, ref, 'twins')
    for b in range(len(B.REPS)):
        assert np.all(ex.counts[b, :2 * n] == 0), b
        want = np.zeros(2 * n)
        want[0::2] = want[1::2] = 0.5 * mult[b] * amb
        assert np.array_equal(av.counts[b, :2 * n], want), b
        assert av.counts[b, :2 * n].sum() == mult[b][amb].sum()
        assert np.array_equal(ex.pi[b, 0:2 * n:2], ex.pi[b, 1:2 * n:2])       # twins keep identical parameters
        assert np.array_equal(ex.counts[b], ref.counts(b, 'exclude')) and np.allclose(av.counts[b], ref.counts(b, 'average'), rtol=RTOL, atol=0)


def test_pooled_state_is_untouched_and_calls_repeat(gpu_device):
    raw = B.case_matrix('C2')
    _, _, _, pp, tp = B.CASES['C2']
    ref = B.case_ref('C2')
    tl = _tl(raw, pp, tp)
    first = tl.bootstrap(len(B.REPS), seed=B.SEED)             # before em()
    B.check_replicates(first, ref, 'before em')
    tl.em()
    z = sp.csr_matrix(tl.z)
    before = (tl.pi.copy(), tl.theta.copy(), tl.lnl, tl.n_iter, z.data.copy(), z.indices.copy(), tl.reassign_colsums('exclude'))
    again = tl.bootstrap(len(B.REPS), seed=B.SEED)
    assert np.array_equal(first.n_iter, again.n_iter) and np.array_equal(first.converged, again.converged)
    assert np.allclose(first.pi, again.pi, rtol=RTOL, atol=0) and np.allclose(first.theta, again.theta, rtol=RTOL, atol=0)
    assert np.allclose(first.lnl, again.lnl, rtol=RTOL, atol=0) and np.array_equal(first.counts, again.counts)
    tl._z = None                                               # export z from the device again
    tl._report_cache = {}
    z2 = sp.csr_matrix(tl.z)
    pi2, theta2 = tl._eng.get_params(1)
    assert np.array_equal(before[0].view(np.uint64), pi2.view(np.uint64)) and np.array_equal(before[1].view(np.uint64), theta2.view(np.uint64))
    assert np.array_equal(before[0], tl.pi) and before[2] == tl.lnl and before[3] == tl.n_iter
    assert np.array_equal(before[4].view(np.uint64), z2.data.view(np.uint64)) and np.array_equal(before[5], z2.indices)
    assert np.array_equal(before[6], tl.reassign_colsums('exclude'))


def test_dropped_column_ids_are_rebuilt_for_the_call_and_dropped_again(gpu_device):
    raw = B.case_matrix('C2')
    _, _, _, pp, tp = B.CASES['C2']
    ref = B.case_ref('C2')
    tl = _tl(raw, pp, tp, drop_csr_indices=1)
    assert tl._eng.device_memory()['resident']['csr_indices'] == 0
    fits = tl.bootstrap(len(B.REPS), seed=B.SEED)
    assert tl._eng.device_memory()['resident']['csr_indices'] == 0
    B.check_replicates(fits, ref, 'drop')
    _check_counts(fits, ref, 'exclude', 'drop')


def test_reproducible_handles_are_refused(gpu_device):
    from telescope_amd._lib import EngineError
    tl = _tl(B.case_matrix('C2'), 1, 5, reproducible=1)
    with pytest.raises(EngineError, match='reproducible'):
        tl.bootstrap(2)


def test_engine_refuses_what_it_cannot_do(gpu_device):
    from telescope_amd import _lib
    tl = _case_tl('C2')
    with pytest.raises(_lib.EngineError):                     # choose, at the C ABI
        tl._eng.bootstrap(2, 0, None, 'choose', 0.9, 1e-7, 10, tl.K)
    raw = B.case_matrix('C2')
    eng = _lib.Engine(gpu_device)                             # a matrix without a model
    eng.load_scores(raw.indptr, raw.indices, raw.data, raw.shape[1], None)
    with pytest.raises(_lib.EngineError) as e:
        eng.bootstrap(2, 0, None, 'exclude', 0.9, 1e-7, 10, raw.shape[1])
    assert e.value.code == _lib.ERR_ARG
    eng.close()
    with pytest.raises(_lib.EngineError):
        tl._eng.set_option('boot_hot_columns', -2)


def test_resume_with_bootstrap_end_to_end(gpu_device, tmp_path, monkeypatch):
    from telescope_amd import cli
    # a single-process command-line run sets TSEM_NO_TORCH for itself (cli.warm_device): in-process here, so it must not stay behind
    # for the rank processes that later tests start (they load torch's HIP runtime first)
    monkeypatch.setenv('TSEM_NO_TORCH', '1')
    ckpt = os.path.join(GOLDEN, 'resume_checkpoint.npz')
    plain, boot = tmp_path / 'plain', tmp_path / 'boot'
    assert cli.main(['resume', ckpt, '--quiet', '--outdir', str(plain)]) == 0
    assert cli.main(['resume', ckpt, '--quiet', '--outdir', str(boot), '--bootstrap', '8', '--bootstrap_seed', '3']) == 0
    assert sorted(os.listdir(str(plain))) == ['telescope-TE_counts.tsv', 'telescope-run_stats.tsv']
    assert sorted(os.listdir(str(boot))) == ['telescope-TE_counts.tsv', 'telescope-bootstrap.tsv', 'telescope-run_stats.tsv']
    for name in ('telescope-TE_counts.tsv', 'telescope-run_stats.tsv'):
        assert (plain / name).read_bytes() == (boot / name).read_bytes(), name
    lines = (boot / 'telescope-bootstrap.tsv').read_text().splitlines()
    head = lines[0].split('\t')
    assert head[0] == '## Bootstrap' and 'replicates:8' in head and 'seed:3' in head and 'method:exclude' in head and 'level:0.95' in head
    assert lines[1].split('\t') == ['transcript', 'count', 'count_mean', 'count_sd', 'count_lo', 'count_hi', 'prop_mean', 'prop_sd',
                                    'prop_lo', 'prop_hi']
    counts = (boot / 'telescope-TE_counts.tsv').read_text().splitlines()
    assert [l.split('\t')[:2] for l in lines[1:]] == [l.split('\t') for l in counts]
    fitted = int([f for f in head if f.startswith('fitted:')][0].split(':')[1])
    assert fitted == 8
    for l in lines[2:]:
        f = l.split('\t')
        mean, sd, lo, hi = (float(x) for x in f[2:6])
        assert lo <= mean <= hi and sd >= 0, l
        pmean, psd, plo, phi = (float(x) for x in f[6:10])
        assert plo <= pmean <= phi and psd >= 0, l
