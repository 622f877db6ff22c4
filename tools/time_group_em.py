"""Per-group EM fits of a few ENORMOUS groups — the cell types of a single-cell run (`sc --pooling_mode celltype`) — through
`TelescopeLikelihood.em_cells` (tsem_cell_em): the spread class (engine option "cell_em_spread_entries": such a group is fitted by the
whole grid, a few short launches per iteration) against one workgroup per group, and against what a caller could do without
em_cells: a loop of one `TelescopeLikelihood(raw[rows_g]).em()` per group, set-up included.

Synthetic droplet run: 5e6 rows x 30 000 loci x ~10 entries per row (zipf columns), every row in one of 20 groups of zipf-distributed
sizes.  em_epsilon 1e-7, max_iter 100, the default priors.  Three runs each, wall clock around synchronised calls, of
  (a) em_cells with the option as the library ships it;
  (b) em_cells with the option at 0 (never spread);
  (l) the loop.
Timed is the call AFTER the first one of a map (the layout is cached per map): the fit alone.  A library that rejects the option —
the commit before the spread class: run this file from a checkout of it — is timed as it is, once: that run is the yardstick (c), and
(b) must agree with it.  Then the sweep that sets the option's default: ONE group of 2^14 ... 2^22 stored entries, spread (option
at 1) and not (option at 0).
    python tools/time_group_em.py [rows=5000000] [groups=20] [runs=3] [loop=1] [sweep_max_log2=22]"""
import logging
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
from telescope_amd import synthetic
from telescope_amd._lib import Engine, EngineError, sources_fingerprint
from telescope_amd.likelihood import TelescopeLikelihood

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
GROUPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
LOOP = int(sys.argv[4]) if len(sys.argv) > 4 else 1
SWEEP_MAX = int(sys.argv[5]) if len(sys.argv) > 5 else 22
K = 30_000
OPTION = 'cell_em_spread_entries'


class O:
    em_epsilon = 1e-7; max_iter = 100; pi_prior = 0; theta_prior = 200000


def rng_str(v):
    return '%.4f - %.4f s (median %.4f)' % (min(v), max(v), float(np.median(v)))


def set_spread(eng, value):
    """False: the library does not know the option (the yardstick run)."""
    try:
        eng.set_option(OPTION, value)
        return True
    except EngineError:
        return False


def timed_fits(tl, cor, n_groups, runs):
    """seconds of `runs` fits after the map's first one (which uploads the map and builds the layout, and warms up), the last fits"""
    tl._eng.set_groups(None, 0)
    fits = tl.em_cells(cor, n_groups)
    out = []
    for _ in range(runs):
        tl._eng.synchronize()
        t0 = time.perf_counter()
        fits = tl.em_cells(cor, n_groups)
        out.append(time.perf_counter() - t0)
    return out, fits


def main():
    logging.basicConfig(level=logging.ERROR)
    eng = Engine(0)
    eng.generate(0, ROWS, K, synthetic.poisson_cdf_u32(10), 42, synthetic.DIST_CODE['zipf'], 0.3)
    tl = TelescopeLikelihood.from_engine(eng, O())
    n, k, nnz = eng.dims()
    rng = np.random.RandomState(2027)
    share = 1.0 / np.arange(1, GROUPS + 1)
    sizes = np.maximum(1, share / share.sum() * ROWS).astype(np.int64)
    sizes[0] += ROWS - sizes.sum()
    cor = np.empty(ROWS, np.int32)
    cor[rng.permutation(ROWS)] = np.repeat(np.arange(GROUPS, dtype=np.int32), sizes)
    known = set_spread(eng, 0)
    print('library sources %s; option "%s" %s' % (sources_fingerprint(), OPTION, 'known' if known else 'NOT known: the yardstick run (c)'))
    print('%d rows x %d loci, %d stored entries; %d groups of %d - %d rows' % (n, k, nnz, GROUPS, sizes.min(), sizes.max()), flush=True)
    ip, ix, rw = eng.export_csr()
    lens = np.diff(ip)
    ne = np.bincount(cor, weights=lens, minlength=GROUPS).astype(np.int64)

    def report(tag, t, fits):
        info = eng.layout_info()
        work = float((ne * fits.n_iter).sum())
        print('%s: fit %s; %.3g entries x iterations/s; iterations %d - %d; classes wave/256/512/global/spread %s'
              % (tag, rng_str(t), work / np.median(t), fits.n_iter.min(), fits.n_iter.max(),
                 [info.get(x, 0) for x in ('cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global', 'cell_em_spread')]), flush=True)

    if not known:
        t_c, fits = timed_fits(tl, cor, GROUPS, RUNS)
        report('(c) em_cells of the library without the spread class', t_c, fits)
    else:
        for tag, value in (('(b) em_cells, option at 0', 0), ('(a) em_cells, option as shipped', None)):
            if value is None:                                # (a fresh handle carries the shipped default)
                tl._eng.close()
                eng = Engine(0)
                eng.generate(0, ROWS, K, synthetic.poisson_cdf_u32(10), 42, synthetic.DIST_CODE['zipf'], 0.3)
                tl = TelescopeLikelihood.from_engine(eng, O())
            t, fits = timed_fits(tl, cor, GROUPS, RUNS)
            report(tag, t, fits)
            if value == 0:
                t_b = t
            else:
                t_a = t
        print('ranges: (a) %.4f - %.4f s, (b) %.4f - %.4f s: %s; ratio of the medians (b) / (a) %.2f'
              % (min(t_a), max(t_a), min(t_b), max(t_b), 'they do not overlap' if max(t_a) < min(t_b) else 'THEY OVERLAP',
                 np.median(t_b) / np.median(t_a)), flush=True)

    if LOOP:
        raw = sp.csr_matrix((rw, ix, ip), shape=(n, k))
        order = np.argsort(cor, kind='stable')
        bounds = np.searchsorted(cor[order], np.arange(GROUPS + 1))
        loop = []
        for _ in range(RUNS):
            t0 = time.perf_counter()
            for g in range(GROUPS):
                one = TelescopeLikelihood(raw[np.sort(order[bounds[g]:bounds[g + 1]])], O())
                one.em()
                one._eng.close()
            loop.append(time.perf_counter() - t0)
        print('(l) loop, one TelescopeLikelihood(raw[rows_g]).em() per group, set-up included: %s' % rng_str(loop), flush=True)
        del raw

    if known and SWEEP_MAX >= 14:
        print('sweep, ONE group of the first rows holding about 2^p stored entries: spread (option at 1) | one workgroup (option at 0)')
        cum = np.cumsum(lens)
        for p in range(14, SWEEP_MAX + 1):
            rows = int(np.searchsorted(cum, 1 << p)) + 1
            if rows > n:
                break
            one = np.full(n, -1, np.int32)
            one[:rows] = 0
            med = []
            for value in (1, 0):
                set_spread(eng, value)
                t, fits = timed_fits(tl, one, 1, RUNS)
                med.append(float(np.median(t)))
                spread_n = eng.layout_info()['cell_em_spread']
                assert spread_n == value, (spread_n, value)
            print('  2^%d: %8d entries, %7d rows, %3d iterations: spread %.5f s | one workgroup %.5f s | ratio %.2f'
                  % (p, int(cum[rows - 1]), rows, int(fits.n_iter[0]), med[0], med[1], med[1] / med[0]), flush=True)
    eng.close()


if __name__ == '__main__':
    main()
