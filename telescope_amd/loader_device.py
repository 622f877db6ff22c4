"""The device loader of `assign` (`--loader device`): loader.load_alignment's dict, key by key, with the per-record work on the GPU.

  host    BGZF inflate (gzip; with inflate='device' the blocks are inflated on the GPU instead: bgzf.DeviceBgzfReader),
          the record chain of every chunk (tsem_bam_scan, C), the cut in front of the chunk's last bundle —
          the last bundle may go on in the next chunk, so it is carried over with the unconsumed tail, and a chunk that holds one
          bundle only grows until a second one begins;
  device  one call per chunk (tsem_bam_chunk, telescope_amd/csrc/tsem_bam.hip): k_bam_decode, k_bam_pair, k_bam_overlap,
          k_bam_fragment -> per bundle the fragment code, the class and the (locus, alnscore, alnlen) list;
  host    first-appearance row ids per name (the same `setdefault`), first-appearance column ids per locus (np.unique per chunk against
          a running table), the counters (np.bincount), the barcode / UMI strings, then loader.mappings_to_result — the Python
          loader's own tail.

A bundle the kernels leave to the host (class 5: more records than `record_cap`, a pair that hits more than 8 loci, a value outside
int32 ...) is decoded with loader.decode_record and run through loader._fragments / assign_pair / score_bundle; its result replaces the
device's at the same position, which makes the load exact for every input.  LAST_STATS holds the last load's counts and wall times.

With `updated_sam` (`--updated_sam --rewrite device`) the two BAMs of the load are written as well: per chunk three more kernels
(tsem_bam_rewrite_size / _fetch, telescope_amd/csrc/tsem_bam_edit.h) turn the chunk into the framed record streams of other.bam and
tmp_tele.bam, the host splices in the records of the bundles it kept (host_bundle(..., streams=True)) and bam_out.BgzfWriter deflates.
"""
import gzip
import io
import logging as lg
import struct
from collections import Counter, OrderedDict
from time import perf_counter

import numpy as np

from . import bam_out
from . import loader as pyl
from ._lib import BAM_STATUS, BamLoader, bam_scan

DEFAULT_CHUNK_BYTES = 64 << 20
CODES = ('SU', 'SM', 'PU', 'PM', 'PX')
CLS_HOST = 5
# rows of BamLoader.chunk's matrix (include/telescope_em.h)
(C_REF, C_POS, C_NREF, C_NPOS, C_ATLEN, C_FLAG, C_LRN, C_NCIG, C_LSEQ, C_AS, C_BITS, C_BCOFF, C_BCLEN, C_UMIOFF, C_UMILEN, C_STATUS,
 C_PAIR1, C_PAIR2, C_BUNDLE, C_PFEAT, C_PAS, C_PLEN, C_MFEAT, C_MAS, C_MLEN, C_BCODE, C_BNPAIRS, C_BNMAPS, C_BCLASS, C_BMIN, C_BMAX,
 C_BNMAPPED, C_BFLAG, C_SCRATCH) = range(34)
BIT_AS, BIT_NEWNAME, BIT_HOST = 1, 2, 4

LAST_STATS = {}
LAST_TMP_TABLE = None
_KIND_OF_SLOT = np.array([0, 0, 0, 2, 1], np.uint8)          # BAM_RW_* (tsem_bam_edit.h) of a tmp slot -> 0 unchanged, 1 SEC, 2 PRI


def annotation_arrays(annotation, refs):
    """The arrays of tsem_bam_open from loader.Annotation._sorted, per BAM reference in header order: (ref_lo, ref_hi, starts, maxend,
    ends, locus, strand, locus names).  The locus ids follow `annotation.loci`."""
    names = list(annotation.loci)
    lid = {n: i for i, n in enumerate(names)}
    ranges, ref_lo, ref_hi = {}, [], []
    starts, maxend, ends, locus, strand = [], [], [], [], []
    n = 0
    for chrom in refs:
        if chrom not in ranges:
            ivs, st, mx = annotation._sorted(chrom)
            ranges[chrom] = (n, n + len(ivs))
            starts.append(st); maxend.append(mx)
            ends.append(np.array([iv[1] for iv in ivs], dtype=np.int64))
            locus.append(np.array([lid[iv[2]] for iv in ivs], dtype=np.int32))
            strand.append(np.array([0 if iv[3] == '+' else (1 if iv[3] == '-' else 2) for iv in ivs], dtype=np.int8))
            n += len(ivs)
        ref_lo.append(ranges[chrom][0]); ref_hi.append(ranges[chrom][1])
    cat = lambda xs, t: np.concatenate(xs).astype(t) if xs else np.zeros(0, t)
    return (np.array(ref_lo, np.int32), np.array(ref_hi, np.int32), cat(starts, np.int64), cat(maxend, np.int64), cat(ends, np.int64),
            cat(locus, np.int32), cat(strand, np.int8), names)


def _same_name(data, a, b):
    l = data[a + 12]
    return l == data[b + 12] and data[a + 36:a + 35 + l] == data[b + 36:b + 35 + l]


def bam_chunks(fh, path, chunk_bytes, max_bundles=None, stats=None):
    """-> (data, rec_off) per chunk of the inflated record stream `fh`: rec_off (int64 [n + 1], tsem_bam_scan) lists whole records that
    form whole bundles; what lies behind rec_off[n] in `data` was carried into the next chunk.  `max_bundles`: at most so many bundles
    per chunk."""
    stats = {} if stats is None else stats
    tail = b''
    while True:
        t0 = perf_counter()
        new = fh.read(chunk_bytes)
        t1 = perf_counter()
        eof = not new
        data = tail + new if tail else new
        off, used = bam_scan(data)
        stats['inflate_s'] = stats.get('inflate_s', 0.) + t1 - t0
        stats['scan_s'] = stats.get('scan_s', 0.) + perf_counter() - t1
        n = len(off) - 1
        cut = n
        if not eof:                                          # the last bundle may go on behind the chunk: it waits for the next one
            cut = n - 1 if n else 0
            while cut > 0 and _same_name(data, int(off[cut - 1]), int(off[cut])):
                cut -= 1
            if cut == 0:                                     # one bundle, or less than a record: the chunk grows
                tail = data
                continue
        elif used != len(data):
            raise ValueError(('%s: truncated BAM record' if len(data) - used < 4 else '%s: truncated BAM') % path)
        if max_bundles:                                      # (tests: [0, cut) in pieces of max_bundles bundles)
            lo = 0
            while lo < cut:
                hi, nb = lo + 1, 1
                while hi < cut:
                    starts_bundle = not _same_name(data, int(off[hi - 1]), int(off[hi]))
                    if starts_bundle and nb == max_bundles:
                        break
                    nb += starts_bundle
                    hi += 1
                base = int(off[lo])
                yield data[base:int(off[hi])], off[lo:hi + 1] - base
                lo = hi
        elif cut:
            yield data, off[:cut + 1]
        if eof:
            return
        tail = data[int(off[cut]):]


def _record_name(data, off, i):
    o, e = int(off[i]), int(off[i + 1])
    l = data[o + 12]
    return data[o + 36:min(o + 35 + l, e)].decode(errors='replace')


def _framed(pairs):
    recs = [r for p in pairs for r in p.records()]
    return b''.join(struct.pack('<i', len(r)) + r for r in recs)


def host_bundle(data, off, s, e, btag, utag, assign, no_feature_key, streams=False):
    """The Python loader's own code on records [s, e) of a chunk (one bundle): dict(code, cls, min, max, maps, bc, umi).  `streams`:
    also what the bundle sends to the BAMs of --updated_sam: other, tmp (framed records) and side = [(kind, ZF | None)] per tmp record
    (kind 0 unchanged, 1 SEC, 2 PRI)."""
    segs = [pyl.decode_record(data[int(off[i]) + 4:int(off[i + 1])], btag, utag, raw=streams) for i in range(s, e)]
    (code, alns), = list(pyl._fragments(iter(segs)))
    r = dict(code=CODES.index(code), cls=0, min=None, max=None, maps=[], bc=None, umi=None, other=b'', tmp=b'', side=[])
    if code in ('SU', 'PU'):
        if streams:
            r['other'], r['n_other'] = _framed(alns[:1]), len(alns[0].records())
        return r
    r['bc'], r['umi'] = alns[0].r1.bc, alns[0].r1.umi
    mapped, _feats, _byfeat, maps = pyl.score_bundle(alns, assign, no_feature_key)
    if mapped:
        r['min'], r['max'] = min(a.alnscore for a in mapped), max(a.alnscore for a in mapped)
    ambig = len(mapped) > 1
    r['cls'] = (2 if ambig else 1) if maps is None else (4 if ambig else 3)
    r['maps'] = maps or []
    if streams and maps is None:
        r['other'], r['n_other'] = _framed(alns), sum(len(p.records()) for p in alns)
    elif streams:
        pyl.tag_bundle(mapped, _byfeat, maps)
        r['tmp'] = _framed(alns)
        for p in alns:
            zt = None if p.is_unmapped else bam_out.get_tag(p.r1.raw, 'ZT')
            r['side'] += [(0, None) if zt is None else (1 if zt == 'SEC' else 2, bam_out.get_tag(p.r1.raw, 'ZF'))] * len(p.records())
    return r


def load_alignment_device(samfile, annotation, no_feature_key='__no_feature', overlap_threshold=0.2, stranded_mode='None',
                          barcode_tag=None, umi_tag=None, device=0, chunk_bytes=None, record_cap=4096, max_bundles=None,
                          on_chunk=None, inflate='host', updated_sam=None, deflate='host', collate='none'):
    """loader.load_alignment(..., loader='device').  `on_chunk(data, rec_off, out)`: called with every chunk's raw device outputs
    (tests); `max_bundles`: at most so many bundles per device call (tests).  `inflate`: 'host' (Python's gzip) or 'device' (the BGZF
    blocks are inflated on the GPU, bgzf.py; a gzip file that is not BGZF is still read by gzip: LAST_STATS['inflate'] says which).
    `updated_sam=(other_bam, tmp_bam)` (rewrite='device'): the two BAMs of the Python loader, byte for byte — per chunk the device
    rewrites the records into two framed streams (tsem_bam_rewrite_size / _fetch), the records of the bundles left to the host are
    spliced in at their bundles' offsets, bam_out.BgzfWriter deflates on the host.  LAST_TMP_TABLE then holds, per record of the tmp
    BAM in order, row (the fragment's row of the matrix, int32), col (the pair's column, int32) and kind (uint8: 0 unchanged, 1 SEC,
    2 PRI) for Telescope.update_sam; it is not part of the returned dict or of the checkpoint.  `deflate='device'`: both writers deflate
    their blocks on the GPU instead (bgzf.DeviceBgzfWriter): the same inflated bytes; LAST_STATS['deflate_blocks'], ['deflate_batches'] and
    ['deflate_ms'] say what went through the device.  `collate`: 'none' (the BAM is name-collated, as the reference asks), 'host' or
    'device': the records behind the header are first brought together by name (collate.py: groups in the order of their first records,
    inside a group the input order), on one host core or on the GPU; LAST_STATS then has 'collate', 'collate_s' and 'collate_ms'.  The
    whole inflated record stream is held in host memory, and for 'device' twice in device memory, during that step."""
    global LAST_STATS, LAST_TMP_TABLE
    LAST_TMP_TABLE = None
    if no_feature_key in annotation.loci:
        raise ValueError('the device loader needs a no_feature_key that is not a locus of the annotation (%r is)' % no_feature_key)
    if inflate not in ('host', 'device'):
        raise ValueError("inflate must be 'host' or 'device', not %r" % (inflate,))
    if deflate not in ('host', 'device'):
        raise ValueError("deflate must be 'host' or 'device', not %r" % (deflate,))
    if collate not in ('none', 'host', 'device'):
        raise ValueError("collate must be 'none', 'host' or 'device', not %r" % (collate,))
    chunk_bytes = DEFAULT_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
    if chunk_bytes < 1:
        raise ValueError('chunk_bytes must be >= 1')
    t_all = perf_counter()
    stats = dict(records=0, bundles=0, chunks=0, fallbacks=0, inflate='host', inflate_fallbacks=0, inflate_s=0., scan_s=0., device_s=0., host_ids_s=0., fallback_s=0., tail_s=0.)
    btag = barcode_tag.encode() if barcode_tag else None
    utag = umi_tag.encode() if umi_tag else None
    if inflate == 'device':
        from .bgzf import DeviceBgzfReader
        fh = DeviceBgzfReader(samfile, device=device)
        stats['inflate'] = fh.inflate
    else:
        fh = io.BufferedReader(gzip.open(samfile, 'rb'), buffer_size=1 << 20)
    dev = w_other = w_tmp = None
    side = ([], [], [])                                      # per chunk: pre-trim row, column, kind of every tmp record
    try:
        refs, _text, _block = pyl.read_bam_header(fh, samfile)
        if collate != 'none':
            from . import collate as col
            fh = col.collated_stream(fh, samfile, collate, device)
            stats.update(collate=collate, collate_s=col.LAST['collate_s'], collate_ms=col.LAST['ms'])
        arrs = annotation_arrays(annotation, refs)
        loc_names = arrs[-1]
        loc_id = {n: i for i, n in enumerate(loc_names)}
        dev = BamLoader(device, *arrs[:-1])
        if updated_sam:
            dev.names(loc_names + [no_feature_key])
            header = dict(text=_text.split(b'\x00', 1)[0].decode(), refs_block=_block)
            w_other = bam_out.BamWriter(updated_sam[0], header, deflate=deflate, device=device)
            w_tmp = bam_out.BamWriter(updated_sam[1], header, deflate=deflate, device=device)
            stats.update(records_other=0, records_tmp=0, bytes_other=0, bytes_tmp=0, rewrite_s=0., splice_s=0., deflate_s=0.)

        def assign(pair):
            return pyl.assign_pair(pair, annotation, refs, stranded_mode, no_feature_key, overlap_threshold)

        info = Counter()
        ridx, fidx = OrderedDict(), OrderedDict([(no_feature_key, 0)])
        col_of = np.full(len(loc_names) + 1, -1, np.int64)   # locus id + 1 -> column; [0]: no locus -> column 0
        col_of[0] = 0
        rows, cols, m_as, m_len = [], [], [], []
        min_as, max_as = pyl.BIG_INT, -pyl.BIG_INT
        read_bc, read_umi = {}, {}
        n_code, n_cls = np.zeros(5, np.int64), np.zeros(6, np.int64)
        for data, off in bam_chunks(fh, samfile, chunk_bytes, max_bundles, stats):
            t0 = perf_counter()
            out, (st, rec) = dev.chunk(data, off, barcode_tag, umi_tag, annotation.run_stranded, stranded_mode, overlap_threshold, record_cap)
            stats['device_s'] += perf_counter() - t0
            n = len(off) - 1
            if st:
                raise ValueError('%s: record %d (%s): %s' % (samfile, stats['records'] + rec, _record_name(data, off, rec),
                                                            BAM_STATUS.get(st, 'status %d' % st)))
            if on_chunk is not None:
                on_chunk(data, off, out)
            starts = np.flatnonzero(out[C_BITS] & BIT_NEWNAME)
            code, cls = out[C_BCODE][starts], out[C_BCLASS][starts].copy()
            nmaps, nmapped = out[C_BNMAPS][starts].copy(), out[C_BNMAPPED][starts].copy()
            # ---- the bundles left to the host: their results go where the device's would be
            t0 = perf_counter()
            hosted = {}
            for bi in np.flatnonzero(cls == CLS_HOST):
                s = int(starts[bi]); e = int(starts[bi + 1]) if bi + 1 < len(starts) else n
                r = host_bundle(data, off, s, e, btag, utag, assign, no_feature_key, streams=w_tmp is not None)
                hosted[int(bi)] = r
                code[bi], cls[bi], nmaps[bi], nmapped[bi] = r['code'], r['cls'], len(r['maps']) if r['cls'] >= 3 else 0, 0
                for k, (_name, f, a, l) in enumerate(r['maps']):
                    if not (-2 ** 31 <= a < 2 ** 31 and l < 2 ** 31):
                        raise OverflowError('signed integer is greater than maximum')     # (what the Python loader's array('i') says)
                    out[C_MFEAT][s + k] = -1 if f == no_feature_key else loc_id[f]
                    out[C_MAS][s + k], out[C_MLEN][s + k] = a, l
                if r['min'] is not None:
                    min_as, max_as = min(min_as, r['min']), max(max_as, r['max'])
            stats['fallbacks'] += len(hosted)
            stats['fallback_s'] += perf_counter() - t0
            t0 = perf_counter()
            n_code += np.bincount(code, minlength=5)
            n_cls += np.bincount(cls, minlength=6)
            have = nmapped > 0
            if have.any():
                min_as = min(min_as, int(out[C_BMIN][starts][have].min()))
                max_as = max(max_as, int(out[C_BMAX][starts][have].max()))
            # ---- names: a row id per fragment with a feature; with tags, barcode / UMI of every fragment that is not unmapped
            lrn = out[C_LRN]
            tagged = barcode_tag or umi_tag
            which = np.flatnonzero(cls >= 1) if tagged else np.flatnonzero(cls >= 3)
            rid = {}
            r1 = out[C_PAIR1]
            for bi in which.tolist():
                s = int(starts[bi]); o = int(off[s]) + 36
                name = data[o:o + int(lrn[s]) - 1].decode()
                if tagged:
                    h = hosted.get(bi)
                    if h is not None:
                        bc, umi = h['bc'], h['umi']
                    else:
                        a = int(r1[s]); oa = int(off[a])
                        bo, bl, uo, ul = int(out[C_BCOFF][a]), int(out[C_BCLEN][a]), int(out[C_UMIOFF][a]), int(out[C_UMILEN][a])
                        bc = data[oa + bo:oa + bo + bl].decode() if bo >= 0 else None
                        umi = data[oa + uo:oa + uo + ul].decode() if uo >= 0 else None
                    if barcode_tag and bc is not None:
                        read_bc[name] = bc
                    if umi_tag and umi is not None:
                        read_umi[name] = umi
                if cls[bi] >= 3:
                    rid[bi] = ridx.setdefault(name, len(ridx))
            # ---- mappings: gather the lists of the fragments with a feature, first-appearance column ids
            fb = np.flatnonzero(cls >= 3)
            if fb.size:
                cnt = nmaps[fb].astype(np.int64)
                first = np.cumsum(cnt) - cnt
                idx = np.repeat(starts[fb], cnt) + (np.arange(int(cnt.sum())) - np.repeat(first, cnt))
                loc = out[C_MFEAT][idx].astype(np.int64)
                u, ui = np.unique(loc, return_index=True)
                new = col_of[u + 1] < 0
                for l in u[new][np.argsort(ui[new], kind='stable')].tolist():
                    col_of[l + 1] = fidx.setdefault(loc_names[l], len(fidx))
                rows.append(np.repeat(np.array([rid[b] for b in fb.tolist()], np.int64), cnt))
                cols.append(col_of[loc + 1].astype(np.int32))
                m_as.append(out[C_MAS][idx]); m_len.append(out[C_MLEN][idx])
            stats['host_ids_s'] += perf_counter() - t0
            if w_tmp is not None:
                # ---- the BAMs of --updated_sam: the device's streams, the hosted bundles' records at their bundles' offsets
                t0 = perf_counter()
                pos_o, pos_t, (st, rec) = dev.rewrite_size(n)
                if st:
                    raise ValueError('%s: record %d (%s): %s' % (samfile, stats['records'] + rec, _record_name(data, off, rec),
                                                                BAM_STATUS.get(st, 'status %d' % st)))
                kind, pslot = dev.rewrite_slots(n)
                s_other, s_tmp = dev.rewrite_fetch(pos_o[n], pos_t[n])
                t1 = perf_counter()
                stats['rewrite_s'] += t1 - t0
                sel = np.flatnonzero(kind >= 2)
                rid_of = np.full(len(starts), -1, np.int64)
                for b, v in rid.items():
                    rid_of[b] = v
                t_kind = _KIND_OF_SLOT[kind[sel]]
                t_row = rid_of[np.searchsorted(starts, out[C_BUNDLE][sel])]
                t_col = np.where(t_kind > 0, col_of[np.maximum(out[C_PFEAT][np.maximum(pslot[sel], 0)].astype(np.int64), -1) + 1], 0)
                stats['records_other'] += int(np.count_nonzero(kind == 1)); stats['records_tmp'] += int(sel.size)
                pieces_o, pieces_t, at_o, at_t = [], [], 0, 0
                ins = ([], [], [], [])
                for bi in sorted(hosted):
                    s, h = int(starts[bi]), hosted[bi]
                    if h['other']:
                        pieces_o += [s_other[at_o:int(pos_o[s])], h['other']]; at_o = int(pos_o[s])
                        stats['records_other'] += h['n_other']
                    if h['tmp']:
                        pieces_t += [s_tmp[at_t:int(pos_t[s])], h['tmp']]; at_t = int(pos_t[s])
                        at = int(np.searchsorted(sel, s))
                        for k, f in h['side']:
                            ins[0].append(at); ins[1].append(rid[bi]); ins[2].append(fidx[f] if k else 0); ins[3].append(k)
                        stats['records_tmp'] += len(h['side'])
                if ins[0]:
                    t_row, t_col, t_kind = np.insert(t_row, ins[0], ins[1]), np.insert(t_col, ins[0], ins[2]), np.insert(t_kind, ins[0], ins[3])
                side[0].append(t_row); side[1].append(t_col); side[2].append(t_kind)
                t2 = perf_counter()
                stats['splice_s'] += t2 - t1
                for p in pieces_o + [s_other[at_o:]]:
                    w_other.write_framed(p); stats['bytes_other'] += len(p)
                for p in pieces_t + [s_tmp[at_t:]]:
                    w_tmp.write_framed(p); stats['bytes_tmp'] += len(p)
                stats['deflate_s'] += perf_counter() - t2
            stats['records'] += n; stats['bundles'] += len(starts); stats['chunks'] += 1
        stats['kernels_ms'] = dev.times()
        if w_tmp is not None:
            stats['rewrite_ms'] = dev.rewrite_times()
        if inflate == 'device':
            stats['inflate_fallbacks'], stats['inflate_blocks'], stats['inflate_ms'] = fh.fallbacks, fh.blocks, fh.times()
    finally:
        fh.close()
        if dev is not None:
            dev.close()
        t0 = perf_counter()
        try:
            if w_other is not None:                          # (a failed load still ends both files with the EOF block)
                w_other.close()
        finally:                                             # (whatever the first close does: the second writer's handles are released too)
            if w_tmp is not None:
                w_tmp.close()
                stats['deflate_s'] += perf_counter() - t0
    if deflate == 'device' and w_other is not None and w_tmp is not None:
        stats['deflate'] = 'device'
        stats.update(bam_out.sum_device_stats([w_other, w_tmp]))
    t0 = perf_counter()
    info['total_fragments'] = int(n_code.sum())
    for c, k in zip(CODES, n_code.tolist()):
        info[c] = k
    info['nofeat_U'], info['nofeat_A'], info['feat_U'], info['feat_A'] = (int(x) for x in n_cls[1:5])
    cat = lambda xs, t: np.concatenate(xs).astype(t, copy=False) if xs else np.zeros(0, t)
    res = pyl.mappings_to_result(annotation, info, ridx, fidx, cat(rows, np.int64), cat(cols, np.int32), cat(m_as, np.int32),
                                 cat(m_len, np.int32), min_as, max_as, read_bc if barcode_tag else None, read_umi if umi_tag else None)
    if updated_sam:                                          # the rows of the tmp records: the ids of the trimmed matrix
        final = np.array([res['read_index'].get(name, -1) for name in ridx], np.int64)
        row = cat(side[0], np.int64)
        LAST_TMP_TABLE = dict(row=np.where(row >= 0, final[row] if final.size else -1, -1).astype(np.int32), col=cat(side[1], np.int32),
                              kind=cat(side[2], np.uint8))
    stats['tail_s'] = perf_counter() - t0
    stats['total_s'] = perf_counter() - t_all
    LAST_STATS = stats
    if stats['inflate_fallbacks']:
        lg.info('device inflate: %d of %d BGZF blocks were left to zlib on the host' % (stats['inflate_fallbacks'], stats['inflate_blocks']))
    if stats.get('deflate') == 'device':
        lg.info('device deflate: %d BGZF blocks of other and tmp_tele in %d batches' % (stats['deflate_blocks'], stats['deflate_batches']))
    if stats['fallbacks']:
        lg.info('device loader: %d of %d fragments were left to the host loader' % (stats['fallbacks'], stats['bundles']))
    lg.debug('device loader: %d records in %d chunks' % (stats['records'], stats['chunks']))
    return res
