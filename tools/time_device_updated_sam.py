"""Time `assign --updated_sam --loader device --rewrite device` on the bundled BAM's record stream tiled K times (tools/time_loader.py's
tiled file).

    python tools/time_device_updated_sam.py [--records 10000000] [--out profiles/r25_device_updated_sam.txt] [--inflate device]

The Python route (load with the two BAMs, then Telescope.update_sam's record loop) runs on one tile for its records/s; the device route
runs on one tile first (warm-up, and its three files are compared with the Python route's, filecmp) and then on the tiled file.
Reported for the load stage and the update stage separately: the rewrite kernels and both copies by HIP events, the host splice, the
host deflate (bam_out.BgzfWriter, zlib level 6), the re-read of the tmp BAM, the whole wall time; the records/s of both routes; and
which stage a user now waits for.
"""
import argparse
import filecmp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
GOLD = os.path.join(ROOT, 'tests', 'golden')


class Opts(object):
    def __init__(self, samfile, gtffile, outdir, **kw):
        self.samfile, self.gtffile, self.outdir, self.exp_tag = samfile, gtffile, outdir, 'telescope'
        self.attribute, self.no_feature_key, self.overlap_mode, self.overlap_threshold = 'locus', '__no_feature', 'threshold', 0.2
        self.stranded_mode, self.reassign_mode, self.conf_prob, self.updated_sam = 'None', 'exclude', 0.9, True
        self.em_epsilon, self.max_iter, self.pi_prior, self.theta_prior, self.use_likelihood = 1e-7, 100, 0, 200000, False
        self.reproducible, self.device, self.version = False, 0, 'timing'
        self.__dict__.update(kw)

    def outfile_path(self, suffix):
        return os.path.join(self.outdir, '%s-%s' % (self.exp_tag, suffix))


def run(opts, ann):
    """load, EM, update_sam -> (Telescope, seconds of the load, of the EM and report, of update_sam)"""
    from telescope_amd import cli
    from telescope_amd.run_container import Telescope
    os.makedirs(opts.outdir, exist_ok=True)
    ts = Telescope(opts)
    t0 = time.perf_counter()
    ts.load_alignment(ann)
    t1 = time.perf_counter()
    np.random.seed(ts.get_random_seed())
    tl, _ = cli.build_model(ts.raw_scores, opts)
    tl.em()
    t2 = time.perf_counter()
    ts.update_sam(tl, opts.outfile_path('updated.bam'), command_line='telescope assign (timing)')
    return ts, t1 - t0, t2 - t1, time.perf_counter() - t2


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--records', type=int, default=10000000, help='at least so many records (whole tiles)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--inflate', default='host', choices=['host', 'device'])
    ap.add_argument('--append', default=None, help='a text file whose lines are put at the end of the report (e.g. the benchmark runs)')
    a = ap.parse_args()
    from time_loader import tiled_bam
    from telescope_amd import _lib, loader, loader_device
    from telescope_amd.run_container import Telescope
    bam, gtf = os.path.join(GOLD, 'bundled_alignment.bam'), os.path.join(GOLD, 'bundled_annotation.gtf')
    ann = loader.Annotation(gtf, 'locus', 'None')
    lines = ['--updated_sam with --loader device --rewrite device, %s' % time.strftime('%Y-%m-%d'), 'sources_fingerprint %s' % _lib.sources_fingerprint()]
    say = lambda s: (lines.append(s), print(s, flush=True))
    dev_kw = dict(loader='device', rewrite='device', inflate=a.inflate, device=a.device)
    status = 0
    with tempfile.TemporaryDirectory() as d:
        po, do = Opts(bam, gtf, os.path.join(d, 'py')), Opts(bam, gtf, os.path.join(d, 'dev'), **dev_kw)
        ts, t_load, _t_em, t_upd = run(po, ann)
        n_tmp_py = sum(1 for _ in loader.read_bam(ts.tmp_bam)[1])
        n1 = sum(1 for _ in loader.read_bam(bam)[1])
        rate_py = (n1 / t_load, n_tmp_py / t_upd)
        say('python route, one tile: load with other.bam and tmp_tele.bam %d records in %.2f s = %.0f records/s; update_sam %d records in %.2f s = '
            '%.0f records/s (profiles/r08_updated_sam.txt: 12,119 and 12,526)' % (n1, t_load, n1 / t_load, n_tmp_py, t_upd, n_tmp_py / t_upd))
        _ts, t_load1, _, t_upd1 = run(do, ann)
        same = all(filecmp.cmp(po.outfile_path(f), do.outfile_path(f), shallow=False) for f in ('other.bam', 'tmp_tele.bam', 'updated.bam'))
        say('device route, one tile (warm-up): load %.3f s, update_sam %.3f s; the three BAMs are the python route\'s files: %s' % (t_load1, t_upd1, same))
        status |= 0 if same else 1
        tiles = -(-a.records // n1)
        path = os.path.join(d, 'tiled.bam')
        t0 = time.perf_counter()
        n = tiled_bam(path, tiles)
        say('input: %d tiles = %d records, %.1f MB compressed (written in %.1f s)' % (tiles, n, os.path.getsize(path) / 1e6, time.perf_counter() - t0))
        big = Opts(path, gtf, os.path.join(d, 'big'), **dev_kw)
        ts, t_load, t_em, t_upd = run(big, ann)
        s, u = loader_device.LAST_STATS, Telescope.LAST_UPDATE_STATS
        sizes = {f: os.path.getsize(big.outfile_path(f)) / 1e6 for f in ('other.bam', 'tmp_tele.bam', 'updated.bam')}
    k, r = s['kernels_ms'], s['rewrite_ms']
    say('device route, load stage: %d records in %.3f s = %.0f records/s; %d to other.bam, %d to tmp_tele.bam; %d chunks; bundles left to the host %d'
        % (s['records'], t_load, s['records'] / t_load, s['records_other'], s['records_tmp'], s['chunks'], s['fallbacks']))
    say('stage                                   seconds')
    rows = [('inflate (read of the stream)', s['inflate_s']), ('scan', s['scan_s']), ('loader kernels and copies (r21)', s['device_s']),
            ('names and ids on the host', s['host_ids_s']), ('rewrite, wall (size, slots, fetch)', s['rewrite_s']),
            ('  k_bam_rw_plan', r['k_bam_rw_plan'] / 1e3), ('  k_bam_rw_size + scans', r['k_bam_rw_size'] / 1e3),
            ('  k_bam_rw_write', r['k_bam_rw_write'] / 1e3), ('  device-to-host (positions, streams)', r['d2h'] / 1e3),
            ('host splice and the update table', s['splice_s']), ('host deflate (BgzfWriter, two files)', s['deflate_s']),
            ('matrix tail', s['tail_s']), ('total', s['total_s'])]
    for name, v in rows:
        say('%-39s %9.4f' % (name, v))
    stream_mb = sum(sizes.values())
    say('EM and nothing else between the stages: %.3f s' % t_em)
    ku = u['kernels_ms']
    say('device route, update stage: %d records in %.3f s = %.0f records/s; %d chunks' % (u['records'], t_upd, u['records'] / t_upd, u['chunks']))
    rows_u = [('tag words: tiles + numpy lookup', u['lookup_s']), ('tmp re-read (inflate + scan)', u['read_s']), ('device, wall (size, fetch)', u['device_s']),
              ('  host-to-device', ku['h2d'] / 1e3), ('  k_bam_upd_size + scan', ku['k_bam_rw_size'] / 1e3), ('  k_bam_rw_write', ku['k_bam_rw_write'] / 1e3),
              ('  device-to-host', ku['d2h'] / 1e3), ('host deflate (BgzfWriter)', u['deflate_s']), ('total', u['total_s'])]
    for name, v in rows_u:
        say('%-39s %9.4f' % (name, v))
    say('files: other.bam %.1f MB, tmp_tele.bam %.1f MB, updated.bam %.1f MB compressed (%.1f MB in all)' % (sizes['other.bam'], sizes['tmp_tele.bam'], sizes['updated.bam'], stream_mb))
    mb = (s['bytes_other'] + s['bytes_tmp'] + u['bytes']) / 1e6
    say('host deflate: %.1f MB of records in %.3f s = %.0f MB/s (one core, zlib level 6)' % (mb, s['deflate_s'] + u['deflate_s'], mb / (s['deflate_s'] + u['deflate_s'])))
    say('rewrite kernels: load stage %.0f MB in %.4f s = %.1f GB/s written; update stage %.0f MB in %.4f s = %.1f GB/s written (a lane per record)'
        % (s['bytes_tmp'] / 1e6 + s['bytes_other'] / 1e6, r['k_bam_rw_write'] / 1e3, (s['bytes_tmp'] + s['bytes_other']) / 1e6 / r['k_bam_rw_write'],
           u['bytes'] / 1e6, ku['k_bam_rw_write'] / 1e3, u['bytes'] / 1e6 / ku['k_bam_rw_write']))
    waits = dict(rows[:5] + rows[9:12] + [('update: ' + x[0], x[1]) for x in rows_u[:3] + rows_u[7:8]])
    worst = max(waits, key=waits.get)
    say('both stages: %.3f s for %d records = %.0f records/s (python route at the one-tile rates: about %.0f s)'
        % (t_load + t_upd, s['records'], s['records'] / (t_load + t_upd), s['records'] / rate_py[0] + u['records'] / rate_py[1]))
    say('the stage a user now waits for: %s, %.3f s; host deflate in all %.3f s of %.3f s' % (worst, waits[worst], s['deflate_s'] + u['deflate_s'], t_load + t_upd))
    if a.append and os.path.exists(a.append):
        lines += open(a.append).read().splitlines()
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return status | (0 if s['fallbacks'] == 0 else 1)


if __name__ == '__main__':
    sys.exit(main())
