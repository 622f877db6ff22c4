"""Time `assign --updated_sam --loader device --rewrite device` with `--deflate device` against `--deflate host` on the bundled BAM's
record stream tiled K times (tools/time_loader.py's tiled file; the rows of profiles/r29_device_deflate.txt).

    python tools/time_device_deflate.py [--records 10000000] [--out FILE] [--inflate device]

Both routes run on one tile first (warm-up; the sizes of the three files against zlib levels 6 and 1 on the same cuts of 0xff00 bytes,
and whether the two routes' files inflate to the same bytes), then on the tiled file, the device route first.  Reported per route:
both stages' wall time and rows; for the device route the deflate row split into upload, k_bgzf_deflate, offsets and pack, download
(HIP events, tsem_bgzf_deflate_times) and the rest, which is the writer's buffer and the file write.
"""
import argparse
import gzip
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
BLOCK = 0xff00


def zlib_size(raw, level):
    """bytes of the BGZF file that zlib at `level` gives for the stream `raw`: frame of 26 per block, the EOF block"""
    return sum(len(zlib.compress(raw[k:k + BLOCK], level)) - 6 + 26 for k in range(0, len(raw), BLOCK)) + 28


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--records', type=int, default=10000000, help='at least so many records (whole tiles)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--inflate', default='host', choices=['host', 'device'])
    a = ap.parse_args()
    from time_device_updated_sam import GOLD, Opts, run
    from time_loader import tiled_bam
    from telescope_amd import _lib, loader, loader_device
    from telescope_amd.run_container import Telescope
    bam, gtf = os.path.join(GOLD, 'bundled_alignment.bam'), os.path.join(GOLD, 'bundled_annotation.gtf')
    ann = loader.Annotation(gtf, 'locus', 'None')
    lines = []
    say = lambda s: (lines.append(s), print(s, flush=True))
    say('--updated_sam --loader device --rewrite device with --deflate device against --deflate host, %s' % time.strftime('%Y-%m-%d'))
    say('sources_fingerprint %s' % _lib.sources_fingerprint())
    kw = dict(loader='device', rewrite='device', inflate=a.inflate, device=a.device)
    with tempfile.TemporaryDirectory() as d:
        one = {}
        for route in ('device', 'host'):
            one[route] = Opts(bam, gtf, os.path.join(d, 'one_' + route), deflate=route, **kw)
            _ts, t_load, _, t_upd = run(one[route], ann)
            say('one tile, --deflate %s: load %.3f s, update_sam %.3f s' % (route, t_load, t_upd))
        for f in ('other.bam', 'tmp_tele.bam', 'updated.bam'):
            x, y = one['host'].outfile_path(f), one['device'].outfile_path(f)
            raw = gzip.open(x).read()
            l6, l1, dev = zlib_size(raw, 6), zlib_size(raw, 1), os.path.getsize(y)
            say('one tile %s: %d bytes inflated; host file %d, zlib level 6 on the cuts %d, level 1 %d, device file %d = %.3f x level 6, %.3f x '
                'level 1; the same inflated bytes: %s' % (f, len(raw), os.path.getsize(x), l6, l1, dev, dev / l6, dev / l1, raw == gzip.open(y).read()))
        n1 = sum(1 for _ in loader.read_bam(bam)[1])
        tiles = -(-a.records // n1)
        path = os.path.join(d, 'tiled.bam')
        t0 = time.perf_counter()
        n = tiled_bam(path, tiles)
        say('input: %d tiles = %d records, %.1f MB compressed (written in %.1f s)' % (tiles, n, os.path.getsize(path) / 1e6, time.perf_counter() - t0))
        for route in ('device', 'host'):
            big = Opts(path, gtf, os.path.join(d, 'big_' + route), deflate=route, **kw)
            _ts, t_load, _t_em, t_upd = run(big, ann)
            s, u = loader_device.LAST_STATS, Telescope.LAST_UPDATE_STATS
            sizes = {f: os.path.getsize(big.outfile_path(f)) / 1e6 for f in ('other.bam', 'tmp_tele.bam', 'updated.bam')}
            say('--deflate %s: load stage %.3f s, update stage %.3f s, both %.3f s' % (route, t_load, t_upd, t_load + t_upd))
            say('  load stage rows: inflate %.3f scan %.3f loader %.3f ids %.3f rewrite %.3f splice %.3f deflate %.3f tail %.3f total %.3f'
                % (s['inflate_s'], s['scan_s'], s['device_s'], s['host_ids_s'], s['rewrite_s'], s['splice_s'], s['deflate_s'], s['tail_s'], s['total_s']))
            say('  update stage rows: lookup %.3f read %.3f device %.3f deflate %.3f total %.3f' % (u['lookup_s'], u['read_s'], u['device_s'], u['deflate_s'], u['total_s']))
            say('  files: other.bam %.1f MB, tmp_tele.bam %.1f MB, updated.bam %.1f MB' % (sizes['other.bam'], sizes['tmp_tele.bam'], sizes['updated.bam']))
            mb = {'load': (s['bytes_other'] + s['bytes_tmp']) / 1e6, 'update': u['bytes'] / 1e6}
            if route == 'device':
                for name, st in (('load', s), ('update', u)):
                    m = st['deflate_ms']
                    dev_s = (m['h2d'] + m['k_bgzf_deflate'] + m['pack'] + m['d2h']) / 1e3
                    say('  %s stage device deflate: %d blocks in %d batches; host-to-device %.4f s, k_bgzf_deflate %.4f s (%.0f MB: %.1f GB/s), offsets and pack '
                        '%.4f s, device-to-host %.4f s; the rest of the row (the writer\'s buffer, the file write) %.4f s'
                        % (name, st['deflate_blocks'], st['deflate_batches'], m['h2d'] / 1e3, m['k_bgzf_deflate'] / 1e3, mb[name],
                           mb[name] / m['k_bgzf_deflate'], m['pack'] / 1e3, m['d2h'] / 1e3, st['deflate_s'] - dev_s))
            else:
                t = s['deflate_s'] + u['deflate_s']
                say('  host deflate: %.1f MB of records in %.3f s = %.0f MB/s (one core, zlib level 6)' % (mb['load'] + mb['update'], t, (mb['load'] + mb['update']) / t))
            for f in sizes:
                os.remove(big.outfile_path(f))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
