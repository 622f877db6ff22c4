"""Time the device loader (`assign --loader device`) on the bundled BAM's record stream tiled K times.

    python tools/time_loader.py [--records 10000000] [--out profiles/r21_device_loader.txt] [--chunk_bytes N] [--inflate device]

Every tile is the bundled file's 66,414 records with four characters of each query name overwritten by the tile's number (numpy, in
place: the records keep their length, the 1,000 fragments of every tile stay distinct from all others), so the load sees K x 1,000
fragments and the timed window is seconds.  One load of the untiled file warms the device up first.  Reported: the whole-load
records/s of the device path, the wall time of each stage (inflate, scan, the device call; inside it host-to-device, each kernel,
device-to-host by HIP events; names and ids on the host, the matrix tail), the Python loader's records/s on one tile, the fallback
count, and the condition of the design: the four kernels plus both copies against zlib's inflate of the same bytes on one core.
`--inflate device`: the same file is then loaded a second time with the BGZF blocks inflated on the GPU (telescope_amd/bgzf.py); the
report holds the inflate stage and the whole load of both paths side by side, and the upload, kernel and download times of
tsem_bgzf_times.
"""
import argparse
import gzip
import io
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden')
DIGITS = np.frombuffer(b'0123456789ABCDEFGHIJKLMNOPQRSTUV', dtype=np.uint8)


def tiled_bam(path, tiles):
    """-> records written.  The bundled stream `tiles` times, the tile number over the four characters behind the name's '/'."""
    from telescope_amd import loader
    from telescope_amd.bam_out import BamWriter
    bam = os.path.join(GOLD, 'bundled_alignment.bam')
    with gzip.open(bam, 'rb') as g:
        raw = g.read()
    fh = io.BytesIO(raw)
    _refs, text, refs_block = loader.read_bam_header(fh, bam)
    body = np.frombuffer(raw[fh.tell():], dtype=np.uint8).copy()
    pos, p = [], 0
    while p < body.size:
        bs = int(body[p:p + 4].view('<i4')[0])
        name = body[p + 36:p + 36 + int(body[p + 12]) - 1].tobytes()
        pos.append(p + 36 + name.index(b'/') + 1)
        p += 4 + bs
    at = np.array(pos, np.int64)[:, None] + np.arange(4)
    w = BamWriter(path, dict(text=text.split(b'\x00', 1)[0].decode(), refs_block=refs_block))
    w._z._level = 1                                          # (the file is read once: fast deflate)
    for t in range(tiles):
        body[at] = DIGITS[[(t >> 15) & 31, (t >> 10) & 31, (t >> 5) & 31, t & 31]]
        w._z.write(body.tobytes())
    w.close()
    return len(pos) * tiles


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--records', type=int, default=10000000, help='at least so many records (whole tiles)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--chunk_bytes', type=int, default=None)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--inflate', default='host', choices=['host', 'device'],
                    help='device: after the load with the host inflate, load the same file again with the device inflate and compare')
    a = ap.parse_args()
    from telescope_amd import _lib, loader, loader_device
    bam, gtf = os.path.join(GOLD, 'bundled_alignment.bam'), os.path.join(GOLD, 'bundled_annotation.gtf')
    ann = loader.Annotation(gtf, 'locus', 'None')
    lines = ['device loader, %s' % time.strftime('%Y-%m-%d'), 'sources_fingerprint %s' % _lib.sources_fingerprint()]
    say = lambda s: (lines.append(s), print(s, flush=True))

    t0 = time.perf_counter()
    want = loader.load_alignment(bam, ann)
    t_py = time.perf_counter() - t0
    got = loader.load_alignment(bam, ann, loader='device', device=a.device)          # warm-up: one chunk
    n1 = loader_device.LAST_STATS['records']
    same = (np.array_equal(got['raw_scores'].indptr, want['raw_scores'].indptr) and np.array_equal(got['raw_scores'].data, want['raw_scores'].data)
            and np.array_equal(got['raw_scores'].indices, want['raw_scores'].indices) and got['run_info'] == want['run_info'])
    say('python loader, one tile: %d records in %.2f s = %.0f records/s (profiles/r08_updated_sam.txt: 12,119)' % (n1, t_py, n1 / t_py))
    say('device loader, one tile (warm-up): %.3f s, equal to the python loader: %s' % (loader_device.LAST_STATS['total_s'], same))

    tiles = -(-a.records // n1)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'tiled.bam')
        t0 = time.perf_counter()
        n = tiled_bam(path, tiles)
        say('input: %d tiles = %d records, %d fragments, %.1f MB compressed (written in %.1f s)'
            % (tiles, n, tiles * want['run_info']['total_fragments'], os.path.getsize(path) / 1e6, time.perf_counter() - t0))
        size_mb = os.path.getsize(path) / 1e6
        t0 = time.perf_counter()
        nbytes = 0
        with gzip.open(path, 'rb') as g:
            while True:
                b = g.read(64 << 20)
                if not b:
                    break
                nbytes += len(b)
        t_inflate = time.perf_counter() - t0
        say('zlib inflate alone, one core: %.1f MB in %.3f s = %.0f MB/s' % (nbytes / 1e6, t_inflate, nbytes / 1e6 / t_inflate))
        t0 = time.perf_counter()
        res = loader.load_alignment(path, ann, loader='device', device=a.device, chunk_bytes=a.chunk_bytes)
        t_dev = time.perf_counter() - t0
        s = loader_device.LAST_STATS
        if a.inflate == 'device':
            t0 = time.perf_counter()
            res2 = loader.load_alignment(path, ann, loader='device', device=a.device, chunk_bytes=a.chunk_bytes, inflate='device')
            t_dev2 = time.perf_counter() - t0
            s2 = loader_device.LAST_STATS
    k = s['kernels_ms']
    say('device loader, whole load: %d records in %.3f s = %.0f records/s; %d rows x %d columns; %d chunks; fallbacks %d'
        % (s['records'], t_dev, s['records'] / t_dev, res['raw_scores'].shape[0], res['raw_scores'].shape[1], s['chunks'], s['fallbacks']))
    say('stage                          seconds')
    for name, v in (('inflate (gzip read)', s['inflate_s']), ('scan (tsem_bam_scan + concat)', s['scan_s']), ('device call, wall', s['device_s']),
                    ('  host-to-device', k['h2d'] / 1e3), ('  k_bam_decode', k['k_bam_decode'] / 1e3), ('  k_bam_pair', k['k_bam_pair'] / 1e3),
                    ('  k_bam_overlap', k['k_bam_overlap'] / 1e3), ('  k_bam_fragment', k['k_bam_fragment'] / 1e3),
                    ('  device-to-host', k['d2h'] / 1e3), ('host fallback bundles', s['fallback_s']), ('names and ids on the host', s['host_ids_s']),
                    ('matrix tail', s['tail_s']), ('total', s['total_s'])):
        say('%-30s %9.4f' % (name, v))
    dev = sum(k[x] for x in ('h2d', 'k_bam_decode', 'k_bam_pair', 'k_bam_overlap', 'k_bam_fragment', 'd2h')) / 1e3
    say('condition: four kernels + both copies = %.4f s  %s  zlib inflate of the same bytes on one core = %.4f s  -> %s'
        % (dev, '<' if dev < t_inflate else '>=', t_inflate, 'met' if dev < t_inflate else 'NOT met'))
    if not dev < t_inflate:
        worst = max(('k_bam_decode', 'k_bam_pair', 'k_bam_overlap', 'k_bam_fragment', 'h2d', 'd2h'), key=lambda x: k[x])
        say('largest device item: %s, %.4f s' % (worst, k[worst] / 1e3))
    host = {x: s[x] for x in ('inflate_s', 'scan_s', 'host_ids_s', 'tail_s')}
    say('largest host stage: %s' % max(host, key=host.get))
    status = 0 if s['fallbacks'] == 0 else 1
    if a.inflate == 'device':
        same = (np.array_equal(res2['raw_scores'].indptr, res['raw_scores'].indptr) and np.array_equal(res2['raw_scores'].data, res['raw_scores'].data)
                and np.array_equal(res2['raw_scores'].indices, res['raw_scores'].indices) and res2['run_info'] == res['run_info'])
        z = s2['inflate_ms']
        say('--inflate device: the same file again, BGZF blocks inflated on the device (%s): equal to the load above: %s'
            % (s2['inflate'], same))
        say('whole load: %d records in %.3f s = %.0f records/s (host inflate: %.3f s); %d BGZF blocks in %d batches; inflate fallbacks %d'
            % (s2['records'], t_dev2, s2['records'] / t_dev2, t_dev, s2['inflate_blocks'], z['batches'], s2['inflate_fallbacks']))
        say('stage                          host inflate   device inflate')
        for name, key in (('inflate (read of the stream)', 'inflate_s'), ('scan (tsem_bam_scan + concat)', 'scan_s'), ('device call, wall', 'device_s'),
                          ('names and ids on the host', 'host_ids_s'), ('matrix tail', 'tail_s'), ('total', 'total_s')):
            say('%-30s %12.4f %16.4f' % (name, s[key], s2[key]))
        dz = (z['h2d'] + z['k_bgzf_inflate'] + z['d2h']) / 1e3
        say('inside the device inflate stage (tsem_bgzf_times): host-to-device %.4f s, k_bgzf_inflate %.4f s, device-to-host %.4f s; '
            'the rest, %.4f s, is the file read, the header walk and the hand-over of the bytes on the host'
            % (z['h2d'] / 1e3, z['k_bgzf_inflate'] / 1e3, z['d2h'] / 1e3, s2['inflate_s'] - dz))
        say('k_bgzf_inflate: %.0f MB/s inflated, %.0f MB/s compressed' % (nbytes / 1e6 / (z['k_bgzf_inflate'] / 1e3),
                                                                          size_mb / (z['k_bgzf_inflate'] / 1e3)))
        say('inflate stage: device %.4f s  %s  host gzip of the same run %.4f s (zlib alone %.4f s)  -> %s'
            % (s2['inflate_s'], '<' if s2['inflate_s'] < s['inflate_s'] else '>=', s['inflate_s'], t_inflate,
               '%.2fx' % (s['inflate_s'] / s2['inflate_s'])))
        if not same or s2['inflate_fallbacks'] or s2['inflate'] != 'device':
            status = 1
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
