"""Per-group bootstrap on the device (`TelescopeLikelihood.bootstrap(..., cell_of_row=...)`, tsem_bootstrap_groups) against the plain
call it extends, on the matrices of tools/time_bootstrap.py: BASELINE config 2 (1M rows x 30 000 loci x ~20 entries per row, uniform
columns) and its zipf variant.  em_epsilon 1e-7, max_iter 100, the default priors; 32 replicates, seed 0.
  (a) tl.bootstrap(32), the unchanged path: wall clock of the synchronised call and the time per batch sweep (wall / sum over the
      batches of their longest replicate).  `plain` as the last argument stops here: the form that also runs on a parent commit.
  (b) the same call with 2 000 and with 100 000 random groups (every row in a group), methods exclude and all: wall clock, the
      difference to (a) per batch and that difference in units of one batch sweep of (a); the first call (which builds the pattern)
      against the cached ones; slots, the longest column list of a group and its search depth, values added per fragment, and the
      device memory of the call: the pattern, the statistics and the batch's accumulators.
Three runs each; ranges (min - max) and medians are printed.
    python tools/time_group_bootstrap.py [rows=1000000] [runs=3] [dists=uniform,zipf] [methods=exclude,all] [plain]"""
import logging
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from telescope_amd import _lib, synthetic
from telescope_amd._lib import Engine
from telescope_amd.likelihood import TelescopeLikelihood

PLAIN = 'plain' in sys.argv[1:]
ARGS = [a for a in sys.argv[1:] if a != 'plain']
ROWS = int(ARGS[0]) if len(ARGS) > 0 else 1_000_000
RUNS = int(ARGS[1]) if len(ARGS) > 1 else 3
DISTS = ARGS[2].split(',') if len(ARGS) > 2 else ['uniform', 'zipf']
METHODS = ARGS[3].split(',') if len(ARGS) > 3 else ['exclude', 'all']
K, NNZ_ROW, REPS, SEED = 30_000, 20.0, 32, 0
GROUPS = (2_000, 100_000)


class O:
    em_epsilon = 1e-7; max_iter = 100; pi_prior = 0; theta_prior = 200000


def rng_str(v, unit='s'):
    return '%.3f - %.3f %s (median %.3f)' % (min(v), max(v), unit, float(np.median(v)))


def timed(tl, **kw):
    tl._eng.synchronize()
    t0 = time.perf_counter()
    fits = tl.bootstrap(REPS, seed=SEED, **kw)
    return time.perf_counter() - t0, fits


def batches(fits):
    return -(-fits.n_rep // fits.info['batch'])


def sweeps(fits):
    """batch sweeps of a call: every batch runs as long as its longest replicate"""
    r = fits.info['batch']
    return int(sum(fits.n_iter[i:i + r].max() for i in range(0, fits.n_rep, r)))


def one_matrix(dist):
    eng = Engine(0)
    eng.generate(0, ROWS, K, synthetic.poisson_cdf_u32(NNZ_ROW), 42, synthetic.DIST_CODE[dist], 0.0)
    tl = TelescopeLikelihood.from_engine(eng, O())
    n, k, nnz = tl._eng.dims()
    print('\n== %s: %d rows x %d loci, %d stored entries ==' % (dist, n, k, nnz), flush=True)
    # ---- (a) ----
    timed(tl)                                                # warm-up (code object, allocator)
    t, plain = [], None
    for _ in range(RUNS):
        a, plain = timed(tl)
        t.append(a)
    a_med, a_min, a_max = float(np.median(t)), min(t), max(t)
    sweep_ms = 1e3 * a_med / sweeps(plain)
    print('(a) bootstrap(%d), batch %d, hot columns %d: %s; iterations %d - %d, %d batches, %d batch sweeps: %.3f ms per batch sweep'
          % (REPS, plain.info['batch'], plain.info['hot_columns'], rng_str(t), plain.n_iter.min(), plain.n_iter.max(), batches(plain),
             sweeps(plain), sweep_ms), flush=True)
    if PLAIN:
        tl._eng.close()
        return
    # ---- (b) ----
    rng = np.random.RandomState(7)
    for g in GROUPS:
        cor = rng.randint(0, g, n).astype(np.int32)
        for method in METHODS:
            if method != 'exclude':
                base = float(np.median([timed(tl, method=method)[0] for _ in range(RUNS)]))
                base_sweeps = sweeps(plain)
            else:
                base, base_sweeps = a_med, sweeps(plain)
            tl._eng.set_groups(None, 0)                      # the next call builds the pattern again
            tl._eng.groups_token = None
            free0 = tl._eng.device_memory()['free']
            first, fits = timed(tl, method=method, cell_of_row=cor, n_cells=g)
            free1 = tl._eng.device_memory()['free']
            t = []
            for _ in range(RUNS):
                b, fits = timed(tl, method=method, cell_of_row=cor, n_cells=g)
                t.append(b)
            med = float(np.median(t))
            c = fits.cells
            longest = int(np.diff(c.group_ptr).max())
            r = fits.info['batch']
            print('(b) %6d groups, %-7s batch %d: %s; first call (builds the pattern) %.3f s: + %.3f s' % (g, method, r, rng_str(t), first, first - med))
            print('      plain call with this method %.3f s: + %.3f ms per batch = %.2f batch sweeps of %.3f ms'
                  % (base, 1e3 * (med - base) / batches(fits), (med - base) / batches(fits) / (base / base_sweeps), 1e3 * base / base_sweeps))
            print('      %d slots, longest column list %d (search depth %d), mean %.1f; values added per fragment %.2f'
                  % (c.nnz, longest, int(np.ceil(np.log2(longest + 1))), c.nnz / float(g), float(np.nansum(fits.counts) / fits.n_frags.sum())))
            print('      device memory: pattern %.1f MB (8 B per group, 4 B per slot) + mean, sd %.1f MB + accumulators %.1f MB (8 B x batch '
                  'per slot, during the call); free memory after the first call against before it (the grouping cached per map, 16 B per '
                  'row, included; an earlier map\'s pattern and statistics released): - %.1f MB'
                  % ((8 * (g + 1) + 4 * c.nnz) / 1e6, 16 * c.nnz / 1e6, 8 * r * c.nnz / 1e6, (free0 - free1) / 1e6), flush=True)
            assert np.array_equal(fits.n_iter, plain.n_iter) and c.n_used == REPS
            if method == 'exclude':
                assert np.array_equal(fits.counts, plain.counts)
    print('ranges of (a): %.3f - %.3f s' % (a_min, a_max))
    tl._eng.close()


def main():
    logging.basicConfig(level=logging.ERROR)
    print('source fingerprint %s; %d replicates, seed %d, %d runs%s' % (_lib.sources_fingerprint(), REPS, SEED, RUNS, '; plain call only' if PLAIN else ''))
    for dist in DISTS:
        one_matrix(dist)


if __name__ == '__main__':
    main()
