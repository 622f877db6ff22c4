"""Bootstrap replicates on the device (`TelescopeLikelihood.bootstrap`, tsem_bootstrap) against what a caller could do before it
existed: per replicate, resample the rows on the host (`np.repeat`), build `TelescopeLikelihood(raw[rows_b])` — upload, set-up and
layout build — and run `.em()`.

BASELINE config 2 (1M rows x 30 000 loci x ~20 entries per row, uniform columns) and its zipf variant (the skewed column
popularity of TE data).  em_epsilon 1e-7, max_iter 100, the default priors; 32 replicates, seed 0, method exclude.
  (a) tl.bootstrap(32) on the resident matrix: wall clock of the synchronised call, the time per replicate-iteration (wall / sum of
      the replicates' iterations) and per batch sweep (wall / sum over the batches of their longest replicate), next to one pooled
      EM iteration of the same matrix (HIP-event time of the EM pass, and wall / iterations of `em()`).
  (b) the A/B that chose the defaults, on the same matrix: boot_hot_columns 0 (every sum a global atomic) against auto, and
      boot_batch 1 / 2 / 4 against 8.
  (c) the host loop, timed on `loop_reps` replicates and scaled to 32 (the CSR is copied to the host once, outside the timing).
Three runs each; ranges (min - max) and medians are printed.
    python tools/time_bootstrap.py [rows=1000000] [runs=3] [loop_reps=8] [dists=uniform,zipf]"""
import logging
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
from telescope_amd import _lib, synthetic
from telescope_amd._lib import Engine
from telescope_amd.likelihood import TelescopeLikelihood

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
RUNS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
LOOP_REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 8
DISTS = sys.argv[4].split(',') if len(sys.argv) > 4 else ['uniform', 'zipf']
K, NNZ_ROW, REPS, SEED = 30_000, 20.0, 32, 0


class O:
    em_epsilon = 1e-7; max_iter = 100; pi_prior = 0; theta_prior = 200000


def rng_str(v, unit='s'):
    return '%.3f - %.3f %s (median %.3f)' % (min(v), max(v), unit, float(np.median(v)))


def model(dist, **options):
    eng = Engine(0)
    for key, value in options.items():
        eng.set_option(key, value)
    eng.generate(0, ROWS, K, synthetic.poisson_cdf_u32(NNZ_ROW), 42, synthetic.DIST_CODE[dist], 0.0)
    return TelescopeLikelihood.from_engine(eng, O())


def timed_bootstrap(tl):
    tl._eng.synchronize()
    t0 = time.perf_counter()
    fits = tl.bootstrap(REPS, seed=SEED)
    return time.perf_counter() - t0, fits


def sweeps(fits):
    """batch sweeps of a call: every batch runs as long as its longest replicate"""
    r = fits.info['batch']
    return int(sum(fits.n_iter[i:i + r].max() for i in range(0, fits.n_rep, r)))


def one_matrix(dist):
    tl = model(dist)
    n, k, nnz = tl._eng.dims()
    print('\n== %s: %d rows x %d loci, %d stored entries ==' % (dist, n, k, nnz), flush=True)
    # ---- the pooled fit: one EM iteration of this matrix ----
    tl.keep_kernel_timing = True
    tl._eng.kernel_stats(reset=True)
    tl._eng.synchronize()
    t0 = time.perf_counter()
    tl.em()
    em_wall = time.perf_counter() - t0
    ks = tl._eng.kernel_stats()
    print('pooled em(): %d iterations in %.3f s: %.3f ms per iteration (wall); EM pass %.3f ms (HIP events, %d launches)'
          % (tl.n_iter, em_wall, 1e3 * em_wall / tl.n_iter, ks['em_ms'] / max(1, ks['em_launches']), ks['em_launches']), flush=True)
    # ---- (a) ----
    timed_bootstrap(tl)                                      # warm-up (code object, allocator)
    t, fits = [], None
    for _ in range(RUNS):
        a, fits = timed_bootstrap(tl)
        t.append(a)
    med = float(np.median(t))
    print('(a) bootstrap(%d), batch %d, hot columns %d: %s' % (REPS, fits.info['batch'], fits.info['hot_columns'], rng_str(t)))
    print('    iterations %d - %d (sum %d), %d converged, %d fitted; %d batch sweeps: %.3f ms per replicate-iteration, %.3f ms per '
          'batch sweep' % (fits.n_iter.min(), fits.n_iter.max(), int(fits.n_iter.sum()), int(fits.converged.sum()), int(fits.fitted.sum()),
                           sweeps(fits), 1e3 * med / fits.n_iter.sum(), 1e3 * med / sweeps(fits)), flush=True)
    boot_t = t
    ip, ix, rw = tl._eng.export_csr()
    tl._eng.close()
    # ---- (b) ----
    for label, options in (('boot_hot_columns 0', {'boot_hot_columns': 0}), ('boot_batch 4', {'boot_batch': 4}),
                           ('boot_batch 2', {'boot_batch': 2}), ('boot_batch 1', {'boot_batch': 1})):
        ab = model(dist, **options)
        timed_bootstrap(ab)
        t, f = [], None
        for _ in range(RUNS):
            a, f = timed_bootstrap(ab)
            t.append(a)
        print('(b) %-18s batch %d, hot columns %4d: %s; %.3f ms per replicate-iteration, %.3f ms per batch sweep'
              % (label + ':', f.info['batch'], f.info['hot_columns'], rng_str(t), 1e3 * np.median(t) / f.n_iter.sum(),
                 1e3 * np.median(t) / sweeps(f)), flush=True)
        assert np.array_equal(f.n_iter, fits.n_iter)
        ab._eng.close()
    # ---- (c) ----
    raw = sp.csr_matrix((rw, ix, ip), shape=(n, k))
    loop = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        for b in range(LOOP_REPS):
            rows = np.repeat(np.arange(n), synthetic.bootstrap_multiplicities(SEED, b, np.arange(n)))
            one = TelescopeLikelihood(raw[rows], O())
            one.em()
            one._eng.close()
        loop.append((time.perf_counter() - t0) * REPS / float(LOOP_REPS))
    print('(c) host loop, %d x (np.repeat, TelescopeLikelihood(raw[rows_b]), em())%s: %s'
          % (REPS, '' if LOOP_REPS == REPS else ', timed on %d replicates and scaled by %g' % (LOOP_REPS, REPS / float(LOOP_REPS)),
             rng_str(loop)))
    print('ratio of the medians, (c) / (a): %.1f x; ranges (a) %.3f - %.3f s, (c) %.3f - %.3f s: %s'
          % (np.median(loop) / np.median(boot_t), min(boot_t), max(boot_t), min(loop), max(loop),
             'they do not overlap' if max(boot_t) < min(loop) else 'THEY OVERLAP'), flush=True)


def main():
    logging.basicConfig(level=logging.ERROR)
    print('source fingerprint %s; %d replicates, seed %d, %d runs' % (_lib.sources_fingerprint(), REPS, SEED, RUNS))
    for dist in DISTS:
        one_matrix(dist)


if __name__ == '__main__':
    main()
