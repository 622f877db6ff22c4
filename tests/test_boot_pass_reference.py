"""No GPU: tests/_boot_pass_reference.py — the exact reference of 1, 2 and 3 iterations of the bootstrap unit that
tests/test_gpu_boot_pass_exact.py holds the kernels to — tied down against `_bootstrap_reference.weighted_fit` (the same closed form
in fp64) and against the oracle on the matrix with repeated rows, within the reference's own derived bounds; and the fairness of
every input the GPU file uses, so that no GPU leg has to skip a row, a column, a replicate or a method."""
import warnings

import numpy as np
import pytest

import _boot_pass_reference as P
import _bootstrap_reference as B

LD = P.LD
SMALL = [('a',), ('a', 225), ('a', 255), ('c',), ('full', 8), ('full', 9), ('k', 1), ('k', 2), ('k', 255), ('k', 256), ('k', 257)]
ALL = SMALL + [('d300',), ('d6000',), ('stop',), ('kbig',)]


def _within(got, want, bound, what, absolute=False):
    frac, j = P.fraction(got, want, bound, absolute)
    assert frac <= 1.0, what + (j, frac)
    return frac


@pytest.mark.parametrize('key', SMALL + [('stop',)], ids=str)
def test_reference_equals_the_weighted_closed_form_in_fp64(key):
    """weighted_fit evaluates the same closed form in fp64 with numpy's own order of additions: within the bounds of the sweeps
    (bincount adds in entry order: any order is allowed for), integer counts equal"""
    c = P.case(*key)
    for t in (1, 2, 3):
        ref = c.ref(t)
        for b, f in enumerate(ref.fits):
            if b > 3:
                break
            for method in P.METHODS:
                with np.errstate(all='ignore'):
                    w = B.weighted_fit(c.raw, c.mult[b], *c.priors, epsilon=0.0, max_iter=t, method=method, thresh=P.CONF)
                what = (key, t, b, method)
                assert w['n_frags'] == f.n_frags and w['n_iter'] == f.n_iter
                if f.n_frags == 0:
                    assert np.isnan(w['pi']).all() and np.isnan(f.pi[-1]).all()
                    continue
                _within(w['pi'], f.pi[-1], f.b_pi[-1], what + ('pi',))
                _within(w['theta'], f.theta[-1], f.b_theta[-1], what + ('theta',))
                _within(w['lnl'], f.lnl, f.lnl_limit, what + ('lnl',), absolute=True)
                if method in P.INT_METHODS:
                    assert np.array_equal(w['counts'], f.counts[method].astype(np.float64)), what
                else:
                    _within(w['counts'], f.counts[method], f.b_counts[method], what + ('counts',))


@pytest.mark.parametrize('key', SMALL, ids=str)
def test_reference_equals_the_oracle_on_repeated_rows(key):
    """OracleModel on raw[np.repeat(arange(N), m)] with max_score = raw.max() at max_iter 1, 2 and 3: the definition of a replicate
    (the stored scores of 0 of leg c's matrix included)"""
    from oracle.telescope_oracle import OracleModel
    c = P.case(*key)
    n = c.raw.shape[0]
    for t in (1, 2, 3):
        ref = c.ref(t)
        for b, f in enumerate(ref.fits):
            if b > 2 or f.n_frags == 0:
                continue
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                om = OracleModel(c.raw[np.repeat(np.arange(n), c.mult[b])], *c.priors, max_score=c.raw.max())
                om.em(0.0, t, False)
                what = (key, t, b)
                assert om.n_iter == f.n_iter
                _within(om.pi, f.pi[-1], f.b_pi[-1], what + ('pi',))
                _within(om.theta, f.theta[-1], f.b_theta[-1], what + ('theta',))
                _within(om.lnl, f.lnl, f.lnl_limit, what + ('lnl',), absolute=True)
                for method in P.METHODS:
                    got = np.asarray(om.reassign(method, P.CONF).sum(0)).ravel().astype(np.float64)
                    if method in P.INT_METHODS:
                        assert np.array_equal(got, f.counts[method].astype(np.float64)), what + (method,)
                    else:
                        _within(got, f.counts[method], f.b_counts[method], what + (method,))


@pytest.mark.parametrize('key', ALL, ids=str)
def test_every_input_of_the_gpu_file_is_fair(key):
    c = P.case(*key)
    eps = {'stop': P.stop_eps, 'kbig': P.kbig_eps}.get(key[0], lambda c: 0.0)(c)
    for t in (1, 2, 3):
        assert c.ref(t, eps).fair() == [], (key, t)
        if eps:
            assert c.ref(t).fair() == [], (key, t, 'epsilon 0')


def test_the_production_matrix_is_fair_at_the_device_sizes():
    """leg b builds its matrix from the device's CU count: 256 (MI355X) and a smaller part, for the formula's sake"""
    for cu in (256, 64):
        assert P.case('b', cu).ref(2).fair() == [], cu


def test_default_draws_are_fair():
    from telescope_amd.synthetic import bootstrap_multiplicities
    c = P.case('a')
    mult = np.stack([bootstrap_multiplicities(11, r, np.arange(c.raw.shape[0])) for r in range(9)])
    for t in (1, 2, 3):
        assert P.BootPass(c.raw, mult, c.priors, t, M=c.M).fair() == [], t


def test_fair_sees_what_it_is_for():
    """a near tie of the two best z, a z at the threshold and a diff at epsilon are reported; an exact tie is not"""
    rows = [(np.array([0, 1]), np.array([300, 300])), (np.array([0, 2]), np.array([300, 299])), (np.array([1]), np.array([200]))]
    raw = P.csr_from_rows(rows, 3)
    mult = np.ones((1, 3), np.uint8)
    ref = P.BootPass(raw, mult, P.PRIORS, 1)
    assert ref.fair() == []                               # row 0 is an exact tie at max_iter = 1
    f = ref.fits[0]
    assert f.assign['exclude'][0] == 0 and f.assign['average'][0] == 0.5
    z = f.z[2]
    assert P.fair(ref.M, ref.fits, 0.0, float(z)) == [('row', 0, 1)]     # a z of row 1 exactly at the threshold
    assert P.fair(ref.M, ref.fits, float(f.diff[1]), P.CONF) == [('stop', 0, 1)]
    # columns 0 and 1 are no twins (column 0 is in row 1 too): after an M-step their parameters differ, and so do the z of row 0
    f2 = P.BootPass(raw, mult, P.PRIORS, 2).fits[0]
    assert f2.z[0] != f2.z[1] and f2.assign['exclude'][:2].sum() == 1


def test_stop_epsilons_do_what_they_are_for():
    c = P.case('stop')
    eps = P.stop_eps(c)
    assert [(f.n_iter, f.converged) for f in c.ref(3, eps).fits][2] == (1, True)
    assert [f.n_iter for f in c.ref(3, eps).fits] == [3, 3, 1, 3, 3, 2, 3, 3]
    f = c.ref(3).fits[5]
    with pytest.raises(ValueError):
        P.eps_for_stop(([np.nan, 1.0, 2.0], [0, 0, 0]), 2)
    assert float(f.diff[2]) < P.eps_for_stop(f, 2) < float(f.diff[1])
    k = P.case('kbig')
    e = P.kbig_eps(k)
    for f in k.ref(3, e).fits:
        assert f.n_iter == 3
        d2 = np.abs(f.pi[2] - f.pi[1])
        assert float(d2[:65536].sum()) < e < float(d2.sum())   # a sum of the first 256 blocks' parts alone would stop in iteration 2


def test_welford_is_mean_and_sd():
    rng = np.random.RandomState(3)
    v = rng.rand(6, 10) * 100
    good = np.array([1, 1, 0, 1, 1, 1], bool)
    mean, sd, k = P.welford(v, good)
    assert k == 5 and np.allclose(mean, v[good].mean(0), rtol=1e-14) and np.allclose(sd, v[good].std(0, ddof=1), rtol=1e-13)
    assert np.isnan(P.welford(v, np.zeros(6, bool))[0]).all() and np.isnan(P.welford(v[:1], [True])[1]).all()


def test_the_group_pattern_and_values():
    c = P.case('a')
    n = c.raw.shape[0]
    for name, grp, G in P.group_maps(n):
        ref = c.ref(1, groups=(grp, G))
        f = ref.fits[0]
        dense = np.zeros((G, c.raw.shape[1]))
        a = f.assign['all'].astype(np.float64) * c.mult[0][c.M.rid]
        for e in np.flatnonzero(grp[c.M.rid] >= 0):
            dense[grp[c.M.rid[e]], c.M.col[e]] += a[e]
        for g in range(G):
            s = slice(f.slot_ptr[g], f.slot_ptr[g + 1])
            assert np.all(np.diff(f.slot_cols[s]) > 0)
            assert np.array_equal(dense[g, f.slot_cols[s]], f.X['all'][s].astype(np.float64)), (name, g)
        assert dense.sum() == f.X['all'].sum()
