"""pytest plug-in: the launch census of the fused kernel (`_lib.Engine.fused_launches`) added up over every engine a test run closes —
which instantiations of k_em_fused a set of tests launches.  profiles/r36_fused_cells.txt section 1 was taken with it:

    python -m pytest -m gpu -p tools.fused_census tests/test_gpu_em_pass_exact.py tests/test_gpu_quad64.py

prints one `FUSED CENSUS` line at the end of the session; FUSED_CENSUS_OUT=<file> also writes [[cell, [n, n_conditional]], ...] as JSON."""
import json
import os

from telescope_amd import _lib

TOTAL = {}
_close = _lib.Engine.close


def _harvest(self):
    if getattr(self, '_h', None):
        try:
            for cell, (n, armed) in self.fused_launches().items():
                t = TOTAL.setdefault(cell, [0, 0])
                t[0] += n
                t[1] += armed
        except _lib.EngineError:
            pass
    _close(self)


_lib.Engine.close = _harvest
_lib.Engine.__del__ = _harvest


def pytest_sessionfinish(session, exitstatus):
    import gc
    gc.collect()
    ran = [c for c, v in TOTAL.items() if v[0] > 0]
    print('\nFUSED CENSUS: %d cells launched unconditionally (%d of them timeline kernels), %d more only with the choice of the lnl form armed'
          % (len(ran), sum(1 for c in ran if c[4]), sum(1 for v in TOTAL.values() if v[0] == 0)))
    out = os.environ.get('FUSED_CENSUS_OUT')
    if out:
        with open(out, 'w') as fh:
            json.dump(sorted([list(c), v] for c, v in TOTAL.items()), fh)
