"""UMI collapse on the device (tsem_umi_dedup, with the upload of the two maps and the copy of the result) against the vectorised
host form of the definition (tests/_umi_reference.py: a bipartite row - (class, column) graph through scipy's connected_components),
on the synthetic 1M rows x 30k loci x ~20 entries matrix with synthetic cells and UMIs: 5000 cells of lognormal sizes, ten UMIs per
fifty fragments of a cell, a tenth of the fragments without barcode and a twentieth without UMI.  Three runs each (range printed);
the two results are compared; the rounds and the workspace come from the library's trace line (TSEM_TRACE, one extra traced call).
    python tools/time_umi_dedup.py [rows=1000000] [reps=3]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np
from telescope_amd import synthetic
from telescope_amd._lib import Engine

ROWS = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
COLS, NNZ_ROW, N_CELLS = 30_000, 20, 5000

eng = Engine(0)
eng.generate(0, ROWS, COLS, synthetic.poisson_cdf_u32(NNZ_ROW), 42, synthetic.DIST_CODE['zipf'], 0.0)
indptr, indices, data = eng.export_csr()
print('%d rows x %d loci, %d stored entries' % (ROWS, COLS, len(indices)), flush=True)
rng = np.random.default_rng(2026)
sizes = np.maximum(1, rng.lognormal(4.5, 1.0, N_CELLS))
cell = rng.choice(N_CELLS, ROWS, p=sizes / sizes.sum()).astype(np.int32)
per_cell = np.bincount(cell, minlength=N_CELLS)
umi = (rng.random(ROWS) * np.maximum(1, per_cell[cell] // 5)).astype(np.int32)      # ~5 fragments per (cell, UMI)
cell[rng.random(ROWS) < 0.10] = -1
umi[rng.random(ROWS) < 0.05] = -1
n_umis = int(umi.max()) + 1

rep, stats = eng.umi_dedup(cell, umi, N_CELLS, n_umis)      # warm-up: code objects, rocPRIM's first launches
dev = []
for _ in range(REPS):
    t0 = time.perf_counter()
    rep, stats = eng.umi_dedup(cell, umi, N_CELLS, n_umis)
    dev.append((time.perf_counter() - t0) * 1e3)
print('stats: %d rows in %d classes, %d components, %d rows dropped' % tuple(stats), flush=True)
print('device (tsem_umi_dedup, upload and result copy included): %.1f - %.1f ms over %d runs' % (min(dev), max(dev), REPS), flush=True)
os.environ['TSEM_TRACE'] = '1'                               # one more call, traced: phases, rounds and workspace on stderr
sys.stderr.flush()
eng.umi_dedup(cell, umi, N_CELLS, n_umis)
del os.environ['TSEM_TRACE']
eng.close()

from _umi_reference import dedup_vectorised  # noqa: E402
host = []
for _ in range(REPS):
    t0 = time.perf_counter()
    hrep, hstats = dedup_vectorised(indptr, indices, data, cell, umi, COLS)
    host.append((time.perf_counter() - t0) * 1e3)
print('host (numpy + scipy connected_components): %.0f - %.0f ms over %d runs' % (min(host), max(host), REPS), flush=True)
print('results equal: %s' % bool(np.array_equal(rep, hrep) and np.array_equal(stats, hstats)), flush=True)
print('host / device: %.1f x (best of each)' % (min(host) / min(dev)), flush=True)
