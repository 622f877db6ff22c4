"""Reference for the per-group bootstrap (`TelescopeLikelihood.bootstrap(..., cell_of_row=...)`, tsem_bootstrap_groups), on top of
`BootRef` (tests/_bootstrap_reference.py): replicate b's per-group values are the oracle's `reassign(method)` matrix of the replicate
— every row repeated as often as its multiplicity says — summed per group; the pattern is structural (the distinct (group, column) of
the grouped rows' stored entries); the statistics are numpy's mean and std (ddof 1) over the good replicates, and a numpy restatement
of Welford's update is held against them on the host.  Shared by tests/test_group_bootstrap_host.py and
tests/test_gpu_group_bootstrap.py."""
import warnings

import numpy as np
import scipy.sparse as sp

from _bootstrap_reference import CONF, RTOL  # noqa: F401


def random_map(seed, n_rows, n_groups, none=0.1, empty=()):
    """A row -> group map from a RandomState of its own: a share `none` of the rows in no group (-1), the groups `empty` without rows."""
    rng = np.random.RandomState(seed)
    live = np.array([g for g in range(n_groups) if g not in empty])
    cor = live[rng.randint(0, len(live), n_rows)].astype(np.int32)
    cor[rng.rand(n_rows) < none] = -1
    return cor


def group_values(ref, b, method, cor, n_cells, thresh=CONF):
    """Dense [n_cells x K]: X_b[g, j] = sum over the replicate's (repeated) rows of group g of the oracle's reassign(method)[row, j]."""
    cor = np.asarray(cor)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = sp.csr_matrix(ref.fits[b].reassign(method, thresh), dtype=np.float64)
    grp = np.repeat(cor, ref.mult[b])
    assert a.shape[0] == len(grp)
    keep = np.flatnonzero(grp >= 0)
    sel = sp.csr_matrix((np.ones(len(keep)), (grp[keep], keep)), shape=(n_cells, len(grp)))
    return np.asarray((sel @ a).todense())


def ungrouped_counts(ref, b, method, cor, thresh=CONF):
    """The column sums of the replicate's rows that are in no group."""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        a = sp.csr_matrix(ref.fits[b].reassign(method, thresh), dtype=np.float64)
    grp = np.repeat(np.asarray(cor), ref.mult[b])
    return np.asarray(a[np.flatnonzero(grp < 0)].sum(0)).ravel()


def structural_pattern(raw, cor, n_cells):
    """(group_ptr int64 [n_cells + 1], cols int32): the distinct (group, column) of the stored entries of the rows with a group,
    ordered by (group, column)."""
    raw = sp.csr_matrix(raw)
    cor = np.asarray(cor)
    k = raw.shape[1]
    g = np.repeat(cor, np.diff(raw.indptr)).astype(np.int64)
    keys = np.unique(g[g >= 0] * k + raw.indices[g >= 0])
    grp, cols = keys // k, (keys % k).astype(np.int32)
    gptr = np.searchsorted(grp, np.arange(n_cells + 1)).astype(np.int64)
    return gptr, cols


def on_pattern(dense, gptr, cols):
    """The values of a dense [n_cells x K] matrix at the pattern's slots."""
    grp = np.repeat(np.arange(len(gptr) - 1), np.diff(gptr))
    return np.asarray(dense)[grp, cols]


def welford(values, good):
    """Welford's update over the rows of `values` [n_rep x n] marked good, in row order — d = x - mean; mean += d / k; M2 += d (x -
    mean) — as the device's fold does it: (mean, sd with ddof 1); mean NaN without a good row, sd NaN below two."""
    values = np.asarray(values, dtype=np.float64).reshape(len(good), -1)
    mean, m2, k = np.zeros(values.shape[1]), np.zeros(values.shape[1]), 0
    for x, ok in zip(values, good):
        if not ok:
            continue
        k += 1
        d = x - mean
        mean = mean + d / k
        m2 = m2 + d * (x - mean)
    nan = np.full(values.shape[1], np.nan)
    return (mean if k else nan), (np.sqrt(m2 / (k - 1)) if k > 1 else nan)


def moments(values, good):
    """numpy's mean and std (ddof 1) over the good rows of `values`; NaN where too few are good."""
    values = np.asarray(values, dtype=np.float64).reshape(len(good), -1)
    v = values[np.asarray(good, dtype=bool)]
    nan = np.full(values.shape[1], np.nan)
    return (v.mean(axis=0) if len(v) else nan), (v.std(axis=0, ddof=1) if len(v) > 1 else nan)


def assert_moments(mean, sd, want_mean, want_sd, label=''):
    """mean / sd against a reference at RTOL, with atol = RTOL x max |mean| (sd is a difference of values of the mean's size)."""
    if np.all(np.isnan(want_mean)):
        assert np.all(np.isnan(mean)) and np.all(np.isnan(sd)), label
        return
    atol = RTOL * float(np.max(np.abs(want_mean))) if len(want_mean) else 0.
    assert np.allclose(mean, want_mean, rtol=RTOL, atol=atol), (label, 'mean')
    assert np.allclose(sd, want_sd, rtol=RTOL, atol=atol, equal_nan=True), (label, 'sd')
