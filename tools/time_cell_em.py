"""Per-cell EM fits in one device call (`TelescopeLikelihood.em_cells`, tsem_cell_em) against what a user could do before it existed:
a Python loop with one `TelescopeLikelihood(raw[rows_c]).em()` per cell — one engine, one layout build and one launch-bound EM each.

Synthetic droplet run: 5e6 rows x 30 000 loci x ~10 entries per row (zipf), 2000 cells of log-normal sizes (90 % of the rows in a
cell).  Both sides fit every cell with em_epsilon 1e-7, max_iter 100, the default priors.
  (a) em_cells: the first call after the map changes (map upload + grouping + per-cell layout + fit) and the call after it (fit
      alone: the layout is cached per map); set-up = the difference.  Then each cell class alone (the other cells' rows in no cell):
      cells/s and entries x iterations/s per class.
  (b) the loop, on the same matrix (CSR copied to the host once, outside the timing).
Three runs each, wall clock around synchronised calls; the ranges (min - max) and the ratio of the medians are printed.
    python tools/time_cell_em.py [rows=5000000] [cells=2000] [runs=3] [loop_cells=all]"""
import logging
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.sparse as sp
from telescope_amd import synthetic
from telescope_amd._lib import Engine
from telescope_amd.likelihood import TelescopeLikelihood

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 5_000_000
CELLS = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
RUNS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
LOOP_CELLS = int(sys.argv[4]) if len(sys.argv) > 4 and sys.argv[4] != 'all' else None
K = 30_000
CLASS_NAMES = ('wave per cell (Kc <= 256, <= 4096 entries)', '256 threads (Kc <= 1024)', '512 threads (Kc <= 3840)',
               '512 threads, global workspace (Kc > 3840)')


class O:
    em_epsilon = 1e-7; max_iter = 100; pi_prior = 0; theta_prior = 200000


def rng_str(v, unit='s'):
    return '%.3f - %.3f %s (median %.3f)' % (min(v), max(v), unit, float(np.median(v)))


def cell_class(kc, ne):
    return np.where((kc <= 256) & (ne <= 4096), 0, np.where(kc <= 1024, 1, np.where(kc <= 3840, 2, 3)))


def timed_fit(tl, cor, n_cells):
    """(seconds of the first call after a new map, seconds of the next call, fits)"""
    tl._eng.set_groups(None, 0)                              # forget the map: the next call uploads it and rebuilds the layout
    tl._eng.synchronize()
    t0 = time.perf_counter()
    tl.em_cells(cor, n_cells)
    t1 = time.perf_counter()
    fits = tl.em_cells(cor, n_cells)
    t2 = time.perf_counter()
    return t1 - t0, t2 - t1, fits


def main():
    logging.basicConfig(level=logging.ERROR)
    eng = Engine(0)
    eng.generate(0, ROWS, K, synthetic.poisson_cdf_u32(10), 42, synthetic.DIST_CODE['zipf'], 0.3)
    tl = TelescopeLikelihood.from_engine(eng, O())
    n, k, nnz = eng.dims()
    rng = np.random.RandomState(2026)
    sizes = rng.lognormal(0.0, 1.0, CELLS)
    sizes = np.maximum(1, sizes * (0.9 * ROWS / sizes.sum())).astype(np.int64)
    cor = np.full(ROWS, -1, np.int32)
    cor[rng.permutation(ROWS)[:int(sizes.sum())]] = np.repeat(np.arange(CELLS, dtype=np.int32), sizes)
    print('%d rows x %d loci, %d stored entries; %d cells, %d rows in a cell (cell sizes %d - %d, median %d)'
          % (n, k, nnz, CELLS, int(sizes.sum()), sizes.min(), sizes.max(), int(np.median(sizes))), flush=True)

    # ---- (a) one device call ----
    timed_fit(tl, cor, CELLS)                                # warm-up (code objects, allocator)
    first, fit = [], []
    for _ in range(RUNS):
        a, b, fits = timed_fit(tl, cor, CELLS)
        first.append(a); fit.append(b)
    setup = [a - b for a, b in zip(first, fit)]
    ip, ix, rw = eng.export_csr()
    raw = sp.csr_matrix((rw, ix, ip), shape=(n, k))
    ne = np.bincount(cor[cor >= 0], weights=np.diff(ip)[cor >= 0], minlength=CELLS).astype(np.int64)
    kc = np.diff(fits.col_ptr)
    work = float((ne * fits.n_iter).sum())
    print('(a) em_cells, all %d cells: first call %s | set-up %s | fit %s' % (CELLS, rng_str(first), rng_str(setup), rng_str(fit)))
    print('    fit: %.0f cells/s, %.3g entries x iterations/s; iterations %d - %d (median %g), %d of %d cells converged'
          % (CELLS / np.median(fit), work / np.median(fit), fits.n_iter.min(), fits.n_iter.max(), float(np.median(fits.n_iter)),
             int(fits.converged.sum()), CELLS), flush=True)
    cls = cell_class(kc, ne)
    for c in range(4):
        sel = np.flatnonzero(cls == c)
        if len(sel) == 0:
            print('    class %d, %s: no cells' % (c, CLASS_NAMES[c]))
            continue
        sub = np.where(np.isin(cor, sel), cor, -1).astype(np.int32)
        timed_fit(tl, sub, CELLS)
        t = [timed_fit(tl, sub, CELLS)[1] for _ in range(RUNS)]
        w = float((ne[sel] * fits.n_iter[sel]).sum())
        print('    class %d, %s: %d cells, %d entries, Kc %d - %d: fit %s; %.0f cells/s, %.3g entries x iterations/s'
              % (c, CLASS_NAMES[c], len(sel), int(ne[sel].sum()), kc[sel].min(), kc[sel].max(), rng_str(t), len(sel) / np.median(t),
                 w / np.median(t)), flush=True)

    # ---- (b) one TelescopeLikelihood per cell ----
    order = np.argsort(cor, kind='stable')
    bounds = np.searchsorted(cor[order], np.arange(CELLS + 1))
    todo = range(CELLS) if LOOP_CELLS is None else range(min(CELLS, LOOP_CELLS))
    loop = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        its = 0
        for c in todo:
            rows = order[bounds[c]:bounds[c + 1]]
            if len(rows) == 0:
                continue
            one = TelescopeLikelihood(raw[rows], O())
            one.em()
            its += one.n_iter
            one._eng.close()
        loop.append(time.perf_counter() - t0)
    scale = CELLS / float(len(todo))
    if scale != 1.0:
        print('(b) timed on the first %d cells and scaled by %.2f to all %d' % (len(todo), scale, CELLS))
        loop = [t * scale for t in loop]
    print('(b) loop, one TelescopeLikelihood(raw[rows_c]).em() per cell: %s; %.1f cells/s' % (rng_str(loop), CELLS / np.median(loop)))
    both = [a for a in first]
    print('ratio of the medians, (b) / (a): %.1f x against the first call (set-up included), %.1f x against the fit alone'
          % (np.median(loop) / np.median(both), np.median(loop) / np.median(fit)))
    print('ranges: (a) first call %.3f - %.3f s, (b) %.3f - %.3f s: %s'
          % (min(both), max(both), min(loop), max(loop), 'they do not overlap' if max(both) < min(loop) else 'THEY OVERLAP'))
    eng.close()


if __name__ == '__main__':
    main()
