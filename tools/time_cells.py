"""Sparse per-barcode counts (tsem_group_counts) against one report pass (tsem_report_colsums) and the dense per-group sums
(tsem_reassign_groups), on the two shapes of the single-cell issue:
  droplet  20M rows x 30k loci x ~8 entries; 10k cells of lognormal sizes (the dense path runs on these alone) and the same cells plus
           200k barcodes of 1-3 fragments (210k x 30k doubles would be 50 GB: no dense path)
  pooled   tools/time_groups.py's shape: 5M rows x 50k loci x ~100 entries, 2000 groups (every group wide)
Wall time per call incl. the host copies of the results (dense: n_groups x K doubles; sparse: 12 B per stored entry), best of `reps`
after one warm-up call.  `choose` is timed with the first best hit of every tied row picked (no host RNG draw).
    python tools/time_cells.py [droplet|pooled|both] [reps=3]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from telescope_amd import synthetic
from telescope_amd._lib import Engine, Z_PREV
from telescope_amd.likelihood import TelescopeLikelihood

METHODS = ('conf', 'all', 'unique', 'exclude', 'choose', 'average')
WHICH = sys.argv[1] if len(sys.argv) > 1 else 'both'
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3


class O:
    em_epsilon = 0.0; max_iter = 3; pi_prior = 0; theta_prior = 200000


def timed(eng, f):
    f()
    eng.synchronize()
    best = float('inf')
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        eng.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best * 1e3


def model(rows, cols, nnz_row, uniq):
    eng = Engine(0)
    eng.generate(0, rows, cols, synthetic.poisson_cdf_u32(nnz_row), 42, synthetic.DIST_CODE['zipf'], uniq)
    tl = TelescopeLikelihood.from_engine(eng, O())
    tl.em()
    _, _, nnz = eng.dims()
    print('%d rows x %d loci, %d stored entries' % (rows, cols, nnz), flush=True)
    return eng, tl


def report(eng):
    ms = timed(eng, lambda: eng.report_colsums(Z_PREV, 0.9))
    print('one report pass (tsem_report_colsums, incl. its host copies)  %9.2f ms' % ms, flush=True)
    return ms


def compare(label, eng, cor, n, dense, rep):
    k = eng.dims()[1]
    t0 = time.perf_counter()
    eng.set_groups(cor, n)
    eng.group_counts('all', 0.9, Z_PREV)                   # (the grouping is built once per map)
    eng.synchronize()
    print('-- %s: %d groups, %d rows in a group; map + grouping + first call %.1f ms'
          % (label, n, int((cor >= 0).sum()), (time.perf_counter() - t0) * 1e3), flush=True)
    out = np.zeros((n, k)) if dense else None
    for method in METHODS:
        nnz = len(eng.group_counts(method, 0.9, Z_PREV)[1])
        ms = timed(eng, lambda: eng.group_counts(method, 0.9, Z_PREV))
        line = '  %-8s sparse %9.2f ms  %6.2f x report  (%10d stored)' % (method, ms, ms / rep, nnz)
        if dense:
            md = timed(eng, lambda: eng.reassign_groups(method, 0.9, Z_PREV, None, n, out=out))
            line += '   dense %9.2f ms (%5.0f MB)  dense / sparse %6.2f' % (md, out.nbytes / 1e6, md / ms)
        print(line, flush=True)


if WHICH in ('droplet', 'both'):
    rows, cols = 20_000_000, 30_000
    print('== droplet shape')
    eng, tl = model(rows, cols, 8, 0.0)
    rng = np.random.RandomState(2026)
    sizes = np.concatenate([np.maximum(1, rng.lognormal(5.5, 1.0, 10_000)).astype(np.int64), rng.randint(1, 4, 200_000)])
    cor = np.full(rows, -1, np.int32)
    cor[rng.permutation(rows)[:int(sizes.sum())]] = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    rep = report(eng)
    compare('10k cells', eng, np.where(cor < 10_000, cor, -1).astype(np.int32), 10_000, True, rep)
    compare('10k cells + 200k barcodes of 1-3 fragments', eng, cor, len(sizes), False, rep)
    eng.close()

if WHICH in ('pooled', 'both'):
    print('== pooled shape')
    eng, tl = model(5_000_000, 50_000, 100, 0.05)
    rep = report(eng)
    compare('2000 pooled groups', eng, np.random.RandomState(11).randint(0, 2000, 5_000_000).astype(np.int32), 2000, True, rep)
    eng.close()
