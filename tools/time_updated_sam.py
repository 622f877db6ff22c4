"""`--updated_sam`: the two timing legs of the feature.
  device  the tag pass (tsem_entry_tags) over rows [0, ROWS) of a generated 50M x 30k x ~40 matrix in tiles of TILE_MB, against
          ONE tsem_rows_lookup (z pass + reassign pass, 16 B written per entry) of the same rows; wall time incl. the host copies,
          best of `reps` after a warm-up
  host    records/s of the rewrite (Telescope.update_sam's loop over the tmp BAM, tag words given) against the loader's records/s
          (load_alignment with updated_sam, which writes the tmp BAM) on the same input; CPU only
    python tools/time_updated_sam.py [device|host|both] [reps=3] [rows=2000000] [bam=tests/golden/bundled_alignment.bam]"""
import os
import sys
import tempfile
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHICH = sys.argv[1] if len(sys.argv) > 1 else 'both'
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 3
ROWS = int(sys.argv[3]) if len(sys.argv) > 3 else 2_000_000
BAM = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, 'tests', 'golden', 'bundled_alignment.bam')
TILE_MB = 256


def best_of(f):
    f()
    best = float('inf')
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return best


def device_leg():
    from telescope_amd import synthetic
    from telescope_amd._lib import Engine, Z_PREV
    from telescope_amd.bam_out import phred_table
    from telescope_amd.likelihood import TelescopeLikelihood

    class O:
        em_epsilon = 0.0; max_iter = 3; pi_prior = 0; theta_prior = 200000
    eng = Engine(0)
    eng.generate(0, 50_000_000, 30_000, synthetic.poisson_cdf_u32(40), 42, synthetic.DIST_CODE['zipf'], 0.3)
    tl = TelescopeLikelihood.from_engine(eng, O())
    tl.em()
    n, k, nnz = eng.dims()
    ip = tl._eng_indptr()
    rows = min(ROWS, n)
    ent = int(ip[rows])
    print('%d rows x %d loci, %d stored entries; timed rows [0, %d): %d entries' % (n, k, nnz, rows, ent), flush=True)
    tab = phred_table()
    which = tl._which(False)
    cap = TILE_MB << 18
    for method in ('exclude', 'conf'):
        def tags():
            r0 = 0
            while r0 < rows:
                r1 = min(rows, max(r0 + 1, int(np.searchsorted(ip, ip[r0] + cap, side='right')) - 1))
                eng.entry_tags(method, 0.9, which, r0, r1, tab, None, n_out=int(ip[r1] - ip[r0]))
                r0 = r1
            eng.entry_tags_end()
        rl = np.arange(rows, dtype=np.int32)
        off = np.ascontiguousarray(ip[:rows + 1])
        t_tags = best_of(tags)
        t_look = best_of(lambda: eng.rows_lookup(method, 0.9, which, rl, off))
        print('device %-8s tag pass %8.1f ms (%5.2f G entries/s, %d tiles of <= %d MB)   rows_lookup %8.1f ms (%5.2f G entries/s)'
              '   ratio %.2f' % (method, t_tags * 1e3, ent / t_tags / 1e9, -(-ent * 4 // (TILE_MB << 20)), TILE_MB, t_look * 1e3,
                                 ent / t_look / 1e9, t_look / t_tags), flush=True)
    eng.close()


def host_leg():
    from telescope_amd import loader
    from telescope_amd.run_container import Telescope

    class Tiles(object):                                   # the device's tag words stand-in: every PRI entry z = 0.5, unassigned
        def __init__(self, n, indptr):
            self.n, self.indptr = n, indptr

        def reassign(self, method, thresh):
            return None

        def entry_tag_tiles(self, method, thresh, assignment=None):
            from telescope_amd.bam_out import tag_word
            w = tag_word(np.full(int(self.indptr[-1]), 0.5), np.zeros(int(self.indptr[-1])))
            yield 0, self.n, w

        def entry_tags(self, r0, r1, *a, **k):
            raise AssertionError('collated input: no row comes back')
        comm = None

    d = tempfile.mkdtemp()

    class O:
        samfile, outdir, exp_tag, no_feature_key, overlap_mode, overlap_threshold = BAM, d, 'telescope', '__no_feature', 'threshold', 0.2
        stranded_mode, reassign_mode, conf_prob, updated_sam, version = 'None', 'exclude', 0.9, True, 'timing'

        def outfile_path(self, suffix):
            return os.path.join(d, 'telescope-%s' % suffix)
    ann = loader.Annotation(os.path.join(ROOT, 'tests', 'golden', 'bundled_annotation.gtf')) if BAM.endswith('bundled_alignment.bam') \
        else loader.Annotation(sys.argv[5])
    n_in = sum(1 for _ in loader.read_bam(BAM)[1])
    ts = Telescope(O())
    t_load = best_of(lambda: ts.load_alignment(ann))
    n_tmp = sum(1 for _ in loader.read_bam(ts.tmp_bam)[1])
    stub = Tiles(ts.raw_scores.shape[0], ts.raw_scores.indptr)
    t_rw = best_of(lambda: ts.update_sam(stub, O().outfile_path('updated.bam'), command_line='timing'))
    print('host   loader (updated_sam on) %d records in %.3f s: %.0f records/s;  rewrite %d records in %.3f s: %.0f records/s'
          '   ratio %.2f' % (n_in, t_load, n_in / t_load, n_tmp, t_rw, n_tmp / t_rw, (n_tmp / t_rw) / (n_in / t_load)), flush=True)


if __name__ == '__main__':
    if WHICH in ('host', 'both'):
        host_leg()
    if WHICH in ('device', 'both'):
        device_leg()
