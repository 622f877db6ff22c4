"""Time the device loader (`assign --loader device`) on the bundled BAM's record stream tiled K times.

    python tools/time_loader.py [--records 10000000] [--out profiles/r21_device_loader.txt] [--chunk_bytes N] [--inflate device]
                                [--collate device]

Every tile is the bundled file's 66,414 records with four characters of each query name overwritten by the tile's number (numpy, in
place: the records keep their length, the 1,000 fragments of every tile stay distinct from all others), so the load sees K x 1,000
fragments and the timed window is seconds.  One load of the untiled file warms the device up first.  Reported: the whole-load
records/s of the device path, the wall time of each stage (inflate, scan, the device call; inside it host-to-device, each kernel,
device-to-host by HIP events; names and ids on the host, the matrix tail), the Python loader's records/s on one tile, the fallback
count, and the condition of the design: the four kernels plus both copies against zlib's inflate of the same bytes on one core.
`--inflate device`: the same file is then loaded a second time with the BGZF blocks inflated on the GPU (telescope_amd/bgzf.py); the
report holds the inflate stage and the whole load of both paths side by side, and the upload, kernel and download times of
tsem_bgzf_times.
`--collate device`: the same records are written a second time in coordinate order (every record of the bundled file sorted by
(ref, pos), the copies of all tiles side by side, as a coordinate sort of the tiled file leaves them) and loaded with `collate='device'`:
the collate stage's wall time and its five HIP-event parts, tsem_bam_collate_host on one core over the same bytes, the whole load
with and without the step, and the gather's bytes/s.
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


def sorted_tiled_bam(path, tiles):
    """-> records written.  The records of tiled_bam(..., tiles) in coordinate order: the bundled file's records sorted by (ref, pos),
    unmapped last, and behind each one its copies in the other tiles (equal position; tile numbers ascending)."""
    from telescope_amd import loader
    from telescope_amd.bam_out import BamWriter
    bam = os.path.join(GOLD, 'bundled_alignment.bam')
    with gzip.open(bam, 'rb') as g:
        raw = g.read()
    fh = io.BytesIO(raw)
    _refs, text, refs_block = loader.read_bam_header(fh, bam)
    body = np.frombuffer(raw[fh.tell():], dtype=np.uint8)
    recs, p = [], 0
    while p < body.size:
        bs = int(body[p:p + 4].view('<i4')[0])
        ref, pos = (int(x) for x in body[p + 4:p + 12].view('<i4'))
        name = body[p + 36:p + 36 + int(body[p + 12]) - 1].tobytes()
        recs.append((ref if ref >= 0 else 1 << 31, pos, p, 4 + bs, 36 + name.index(b'/') + 1))
        p += 4 + bs
    recs.sort(key=lambda r: r[:2])
    t = np.arange(tiles)
    digits = DIGITS[np.stack([(t >> 15) & 31, (t >> 10) & 31, (t >> 5) & 31, t & 31], axis=1)]
    w = BamWriter(path, dict(text=text.split(b'\x00', 1)[0].decode(), refs_block=refs_block))
    w._z._level = 1
    batch, held = [], 0
    for _ref, _pos, at, size, name_at in recs:
        block = np.tile(body[at:at + size], (tiles, 1))
        block[:, name_at:name_at + 4] = digits
        batch.append(block.tobytes()); held += block.size
        if held >= 16 << 20:
            w._z.write(b''.join(batch)); batch, held = [], 0
    w._z.write(b''.join(batch))
    w.close()
    return len(recs) * tiles


def collate_report(path, ann, a, say, res, t_plain):
    """the --collate device part of the report: `path` is the coordinate-sorted file, res / t_plain the load of the name-ordered one"""
    from telescope_amd import _lib, collate, loader, loader_device
    t0 = time.perf_counter()
    res3 = loader.load_alignment(path, ann, loader='device', device=a.device, chunk_bytes=a.chunk_bytes, collate='device', inflate=a.inflate)
    t_col = time.perf_counter() - t0
    s3, c = dict(loader_device.LAST_STATS), dict(collate.LAST)
    ms = c['ms']
    same = res3['run_info'] == res['run_info'] and res3['raw_scores'].shape == res['raw_scores'].shape and res3['raw_scores'].nnz == res['raw_scores'].nnz
    say('--collate device: the same records in coordinate order: %d records, %d names, %d records moved; run_info, shape and stored '
        'entries equal to the load of the name-ordered file: %s' % (c['records'], c['names'], c['moved'], same))
    say('whole load with the step (inflate %s): %.3f s = %.0f records/s; the name-ordered file without it (inflate %s): %.3f s'
        % (a.inflate, t_col, c['records'] / t_col, a.inflate, t_plain))
    say('collate stage, wall (scan, the call, the copy of the result): %.4f s; reading the whole stream in front of it: %.4f s'
        % (c['collate_s'], c['read_s']))
    for name in ('h2d', 'hash_insert_key', 'sort_scan', 'gather', 'd2h'):
        say('  %-28s %9.4f' % (name, ms[name] / 1e3))
    with gzip.open(path, 'rb') as g:
        raw = g.read()
    fh = io.BytesIO(raw)
    loader.read_bam_header(fh, path)
    data = raw[fh.tell():]
    del raw
    off, _used = _lib.bam_scan(data)
    t0 = time.perf_counter()
    h_out, h_order, h_names, _ = _lib.bam_collate(data, off, device=None)
    t_host = time.perf_counter() - t0
    d_out, d_order, d_names, ms2 = _lib.bam_collate(data, off, device=a.device)
    equal = bool(np.array_equal(h_order, d_order) and h_names == d_names and np.array_equal(h_out, d_out))
    dev = sum(ms.values()) / 1e3
    say('tsem_bam_collate_host, one core, the same %.1f MB: %.3f s; tsem_bam_collate (five parts): %.3f s = %.1fx; equal bytes, order '
        'and names: %s' % (len(data) / 1e6, t_host, dev, t_host / dev, equal))
    say('second call on the warm device (five parts): %s' % ', '.join('%s %.4f' % (k, v / 1e3) for k, v in ms2.items()))
    g = 2 * len(data) / (ms2['gather'] / 1e3) / 1e9
    say('k_collate_gather: %.1f MB read and as many written in %.4f s = %.0f GB/s (a streaming read on this chip: about 6,500 GB/s, '
        'profiles/r02_stream_ubench.log)' % (len(data) / 1e6, ms2['gather'] / 1e3, g))
    return 0 if same and equal and s3['fallbacks'] == 0 else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--records', type=int, default=10000000, help='at least so many records (whole tiles)')
    ap.add_argument('--out', default=None, help='also write the report to this file')
    ap.add_argument('--chunk_bytes', type=int, default=None)
    ap.add_argument('--device', type=int, default=0)
    ap.add_argument('--inflate', default='host', choices=['host', 'device'],
                    help='device: after the load with the host inflate, load the same file again with the device inflate and compare')
    ap.add_argument('--collate', default='none', choices=['none', 'device'],
                    help='device: write the same records in coordinate order as well and load them with collate=device')
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
    if a.collate == 'device':
        with tempfile.TemporaryDirectory() as d:
            spath = os.path.join(d, 'sorted.bam')
            t0 = time.perf_counter()
            sorted_tiled_bam(spath, tiles)
            print('coordinate-sorted input written in %.1f s' % (time.perf_counter() - t0), flush=True)
            status = collate_report(spath, ann, a, say, res, t_dev2 if a.inflate == 'device' else t_dev) or status
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
