#!/usr/bin/env python3
"""`--updated_sam` fixture: what the REFERENCE writes for the updated alignment file, and a small BAM built to stress it.

DEV-CONTAINER ONLY (imports /root/reference through tools/make_loader_fixture.py and tools/ref_import.py).  Writes
    tests/golden/updated_mixed.bam / .gtf   a small name-collated BAM: exact best-hit ties (four and eight loci of equal support, so
                                            z = 0.25 / 0.125 — an XP rounding tie), mates split across pairs in a proper-pair bundle,
                                            unmapped mates in PX fragments, records that already carry XP / YC (and a B-array ZB),
                                            a SEC alignment, a score tie between loci, no-overlap and unmapped (two-record SU) bundles
    tests/golden/updated_sam_expected.json  per input (loader_mixed, sc_mixed, updated_mixed, bundled) and reassign mode: the records
                                            of -other.bam, -tmp_tele.bam and -updated.bam as canonical text (qname, flag, MAPQ, every
                                            tag as NAME:TYPE:VALUE in order); for the bundled BAM their SHA-256 instead
    tests/golden/updated_sam_expected.npz   per input and mode: the reference's z (`tl.z[i, j]`) and assignment (`mat[i, j]`) at every
                                            stored entry of the raw score matrix — what a host test feeds the record rewrite

What produces the expectations: the reference's own `Telescope.load_alignment` / `_load_sequential` (model.py:155-285, with
`process_overlap_frag`, model.py:30-63), `_mapping_to_matrix`, `TelescopeLikelihood.em`, `output_report` (bulk or scTelescope, so that
`choose` consumes numpy's legacy stream as a run does) and `update_sam` (model.py:479-521), imported from /root/reference and run
UNMODIFIED on the pysam-named stubs below: `AlignmentFile` (read a BAM, write records — a snapshot at the time of writing — and
re-read what was written), `AlignedSegment` with pysam's `set_tag` (the old tag is deleted, the new one APPENDED; a Python int gets
the smallest integer type that holds it: C S I, c s i below 0; a str Z), `flag`, `mapping_quality`, `has_tag` / `get_tag`, and the
pair methods `write`, `set_mapq`, `set_flag`, `unset_flag` of the unbuildable Cython `AlignedPair`.  The header's `@PG` append
(model.py:488-492) goes to a throw-away list (pysam >= 0.19 edits a copy).  The BAM parser and encoder here are data
tooling, not reference material.
"""
import copy
import gzip
import hashlib
import json
import os
import re
import struct
import sys
import tempfile
from collections import Counter, OrderedDict, defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import make_loader_fixture as L  # noqa: E402

GOLD = L.GOLD
VERSION = '1.0.3.1-mi355x'
MODES = ('exclude', 'choose', 'average', 'conf', 'unique')
PAIRED, PROPER, UNMAP, MUNMAP, REV, MREV, R1, R2, SECONDARY = L.PAIRED, L.PROPER, L.UNMAP, L.MUNMAP, L.REV, L.MREV, L.R1, L.R2, L.SECONDARY

# ------------------------------------------------------------------------------------------------------------ the small BAM
GTF_ROWS = [('chrA', 1000 + 2000 * i, 1999 + 2000 * i, '+', 'T%d' % (i + 1)) for i in range(8)] + \
           [('chrB', 100, 900, '+', 'U1'), ('chrB', 5000, 5600, '-', 'U2')] + \
           [('chrB', 10000 + 4000 * i, 10999 + 4000 * i, '+', 'V%d' % (i + 1)) for i in range(8)]
OLD = b'XPZold\x00YCZ0,0,0\x00'                               # tags an input may already carry


def T(i, off=100):                                            # a position inside locus T<i>
    return 1000 + 2000 * (i - 1) + off


def build_records():
    rec, pair = L.rec, L.pair
    R = []
    for f in range(3):                                        # 8-way exact ties on eight loci nothing else hits: z = 1/8 each
        q = 'h%02d' % f
        R += [rec(q, 0 if i == 0 else SECONDARY, 1, 10100 + 4000 * i, '50M', -4) for i in range(8)]
    for f in range(4):                                        # 4-way exact ties
        q = 't%02d' % f
        R += [rec(q, 0 if i == 1 else SECONDARY, 0, T(i, 300), '50M', -2) for i in range(1, 5)]
    R += [rec('u01', 0, 1, 200, '50M', 0), rec('u02', 0, 1, 300, '40M', -1), rec('u03', REV, 1, 5100, '50M', -3)]
    R[-1]['tags'] = OLD                                       # unique, with an old XP / YC
    # proper-pair bundle whose second alignment's mates do not match: one pair + two lone reads
    R += pair('k01', 0, T(1, 500), '50M', -1, T(1, 700), '50M', -1, 250)
    R += [rec('k01', PAIRED | PROPER | R1 | MREV | SECONDARY, 0, T(2, 500), '50M', -1, 0, T(2, 700), 250),
          rec('k01', PAIRED | PROPER | R2 | REV | SECONDARY, 0, T(2, 750), '50M', -1, 0, T(2, 500), -250)]
    for r in R[-4:]:
        r['tags'] = OLD
    # PX: read 1 mapped twice (T5, T6), read 2 unmapped (with old tags)
    R += [rec('p01', PAIRED | MUNMAP | R1, 0, T(5), '50M', -5, 0, T(5), 0),
          rec('p01', PAIRED | MUNMAP | R1 | SECONDARY, 0, T(6), '50M', -5, 0, T(6), 0),
          rec('p01', PAIRED | UNMAP | R2, 0, T(5), '', None, 0, T(5), 0)]
    R[-1]['tags'] = OLD
    R += [rec('p02', PAIRED | R1, 0, T(7), '50M', -2, 1, 300, 0),
          rec('p02', PAIRED | R2 | REV, 1, 300, '50M', -2, 0, T(7), 0)]                 # PX improper, two hits
    R += [rec('s01', 0, 0, T(3, 600), '50M', -9), rec('s01', SECONDARY, 0, T(3, 650), '50M', -1),
          rec('s01', SECONDARY, 0, T(4, 650), '30M', -1)]      # SEC in T3; a score tie T3 / T4 of different lengths
    for r in R[-3:]:
        r['tags'] = OLD
    R += [rec('n01', 0, 0, 60000, '50M', -1)]                 # no overlap
    R += [rec('x01', UNMAP), rec('x01', UNMAP)]               # SU with two records: only the first goes to -other.bam
    R += [rec('h99', 0, 0, T(8), '50M', -4)]                  # unique on T8
    return R


def bam_bytes(records):
    out = bytearray(b'BAM\x01')
    text = '@HD\tVN:1.6\tSO:unsorted\tGO:query\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % r for r in L.REFS) + \
        '@PG\tID:telescope\tPN:aligner\n'                     # an ID the updated file's @PG line must not reuse
    out += struct.pack('<i', len(text)) + text.encode() + struct.pack('<i', len(L.REFS))
    for name, ln in L.REFS:
        out += struct.pack('<i', len(name) + 1) + name.encode() + b'\x00' + struct.pack('<i', ln)
    for r in records:
        cig = [(int(n), L.OPS[o]) for n, o in re.findall(r'(\d+)([MIDNSHP=X])', r['cigar'])]
        l_seq = sum(n for n, o in cig if o in (0, 1, 4, 7, 8)) or 30
        qn = r['qname'].encode() + b'\x00'
        body = struct.pack('<iiBBHHHiiii', r['ref_id'], r['pos'], len(qn), 30, 4680, len(cig), r['flag'], l_seq,
                           r['nref'], r['npos'], r['tlen'])
        body += qn + b''.join(struct.pack('<I', (n << 4) | o) for n, o in cig)
        body += bytes([0x11] * ((l_seq + 1) // 2)) + bytes([30] * l_seq)
        if r['AS'] is not None:
            body += b'ASi' + struct.pack('<i', r['AS'])
        body += r.get('tags', b'ZBBs' + struct.pack('<ihh', 2, 1, 2))
        out += struct.pack('<i', len(body)) + body
    return bytes(out)


# --------------------------------------------------------------------------------------------- pysam-named stubs
_FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I', 'f': '<f'}


def _int_type(v):
    if v >= 0:
        return 'C' if v <= 0xff else ('S' if v <= 0xffff else 'I')
    return 'c' if v >= -0x80 else ('s' if v >= -0x8000 else 'i')


class Seg(object):
    """pysam.AlignedSegment as far as the reference's loader and update_sam use it"""
    def __init__(self, d, refs):
        self.__dict__.update(d)
        self.reference_name = refs[self.reference_id] if self.reference_id >= 0 else None
    is_paired = property(lambda s: bool(s.flag & PAIRED))
    is_proper_pair = property(lambda s: bool(s.flag & PROPER))
    is_unmapped = property(lambda s: bool(s.flag & UNMAP))
    is_reverse = property(lambda s: bool(s.flag & REV))
    is_read1 = property(lambda s: bool(s.flag & R1))
    is_read2 = property(lambda s: bool(s.flag & R2))

    def get_blocks(self):
        out, pos = [], self.reference_start
        for ln, op in self.cigar:
            if op in (0, 7, 8):
                out.append((pos, pos + ln)); pos += ln
            elif op in (2, 3):
                pos += ln
        return out

    def has_tag(self, t):
        return any(n == t for n, _, _ in self.tags)

    def get_tag(self, t):
        for n, _, v in self.tags:
            if n == t:
                return v
        raise KeyError(t)

    def get_tags(self):
        return [(n, v) for n, _, v in self.tags]

    def set_tag(self, t, v, value_type=None, replace=True):
        self.tags = [x for x in self.tags if x[0] != t]
        if isinstance(v, str):
            typ = 'Z'
        elif isinstance(v, (int, np.integer)):
            v = int(v)
            typ = _int_type(v)
        else:
            raise TypeError(v)
        self.tags.append((t, typ, v))

    def text(self):
        tags = ['%s:%s:%s' % (n, typ, v) for n, typ, v in self.tags]
        return '\t'.join([self.query_name, str(self.flag), str(self.mapping_quality)] + tags)


def parse_bam(path):
    data = gzip.open(path, 'rb').read()
    (l_text,) = struct.unpack_from('<i', data, 4)
    p = 8 + l_text
    (n_ref,) = struct.unpack_from('<i', data, p); p += 4
    refs = []
    for _ in range(n_ref):
        (ln,) = struct.unpack_from('<i', data, p)
        refs.append(data[p + 4:p + 4 + ln - 1].decode()); p += 8 + ln
    out = []
    while p < len(data):
        (bs,) = struct.unpack_from('<i', data, p)
        b = data[p + 4:p + 4 + bs]; p += 4 + bs
        ref, pos, l_rn, mq, _bin, n_cig, flag, l_seq, nref, npos, tlen = struct.unpack_from('<iiBBHHHiiii', b, 0)
        q = 32
        name = b[q:q + l_rn - 1].decode(); q += l_rn
        cig = [(c >> 4, c & 0xF) for c in struct.unpack_from('<%dI' % n_cig, b, q)]; q += 4 * n_cig
        q += (l_seq + 1) // 2 + l_seq
        tags = []
        while q < bs:
            t, typ = b[q:q + 2].decode(), chr(b[q + 2]); q += 3
            if typ in _FMT:
                (v,) = struct.unpack_from(_FMT[typ], b, q); q += struct.calcsize(_FMT[typ])
                v = repr(v) if typ == 'f' else v
            elif typ == 'A':
                v = chr(b[q]); q += 1
            elif typ in 'ZH':
                e = b.index(b'\x00', q); v = b[q:e].decode(); q = e + 1
            else:
                sub = chr(b[q]); (cnt,) = struct.unpack_from('<i', b, q + 1)
                vals = struct.unpack_from('<%d%s' % (cnt, _FMT[sub][1]), b, q + 5)
                v = sub + ',' + ','.join(str(x) for x in vals); q += 5 + cnt * struct.calcsize(_FMT[sub])
            tags.append((t, typ, v))
        out.append(dict(query_name=name, flag=flag, reference_id=ref, reference_start=pos, next_reference_id=nref,
                        next_reference_start=npos, template_length=tlen, mapping_quality=mq, cigar=cig, tags=tags))
    return refs, out


WRITTEN = {}                                                   # path -> [record snapshots], what the stub AlignmentFile wrote


class AlignmentFile(object):
    def __init__(self, path, mode='r', check_sq=False, template=None, header=None):
        self.path, self.mode = path, mode
        if 'w' in mode:
            self.refs = (template.refs if template is not None else None)
            WRITTEN[path] = []
        elif path in WRITTEN:
            self.refs = WRITTEN[path + '#refs']
        else:
            self.refs, self._recs = parse_bam(path)
        self.header = {'PG': []}

    def fetch(self, until_eof=True, **kw):
        src = WRITTEN[self.path] if self.path in WRITTEN else self._recs
        return iter([Seg(copy.deepcopy(d), self.refs) for d in src])

    def write(self, seg):
        d = {k: copy.deepcopy(v) for k, v in seg.__dict__.items() if k != 'reference_name'}
        WRITTEN[self.path].append(d)
        return 1

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class AlignedPair(L.AlignedPair):
    """the pair methods of calignment.pyx that update_sam and the loader call (the Cython module cannot be built here)"""
    def write(self, outfile):
        n = outfile.write(self.r1)
        if self.r2 is not None:
            n += outfile.write(self.r2)
        return n

    def set_mapq(self, value):
        for r in (self.r1, self.r2):
            if r is not None:
                r.mapping_quality = value

    def set_flag(self, b):
        for r in (self.r1, self.r2):
            if r is not None:
                r.flag = r.flag | b

    def unset_flag(self, b):
        for r in (self.r1, self.r2):
            if r is not None:
                r.flag = r.flag & ~b


class GtfAnnotation(L.BruteAnnotation):
    """L.BruteAnnotation over a GTF file, bucketed by chromosome and 10 kb bins (the bundled annotation has thousands of exons)"""
    def __init__(self, gtf):
        rows = []
        for line in open(gtf):
            f = line.rstrip('\n').split('\t')
            if line.startswith('#') or len(f) < 9 or f[2] != 'exon':
                continue
            attr = dict(re.findall(r'(\w+)\s+"(.+?)";', f[8]))
            if 'locus' in attr:
                rows.append((f[0], int(f[3]), int(f[4]), f[6], attr['locus']))
        super().__init__(rows, 'None')
        self.loci = OrderedDict((r[4], None) for r in rows)
        self.bins = defaultdict(list)
        for iv in self.ivs:
            for b in range(iv[1] // 10000, (iv[2] - 1) // 10000 + 1):
                self.bins[(iv[0], b)].append(iv)

    def intersect_blocks(self, ref, blocks, frag_strand):
        res = Counter()
        for bs, be in blocks:
            qb, qe = bs, be + 1
            seen = set()
            for b in range(qb // 10000, (qe - 1) // 10000 + 1):
                for iv in self.bins.get((ref, b), ()):
                    if id(iv) in seen:
                        continue
                    seen.add(id(iv))
                    chrom, s, e, loc, strand = iv
                    if s < qe and qb < e:
                        res[loc] += min(e, qe) - max(s, qb)
        return res


# --------------------------------------------------------------------------------------------------------- the runs
def reference_run(bam, gtf, mode, sc, outdir):
    from telescope.utils import alignment, model
    from telescope.utils.model import Telescope, TelescopeLikelihood, scTelescope
    from telescope.utils.sparse_plus import csr_matrix_plus

    class Opts(object):
        samfile, updated_sam, no_feature_key, overlap_mode, overlap_threshold = bam, True, L.NOFEAT, 'threshold', 0.2
        stranded_mode, ncpu, reassign_mode, conf_prob, use_every_reassign_mode = 'None', 1, mode, 0.9, False
        pi_prior, theta_prior, em_epsilon, max_iter, use_likelihood, barcode_tag = 0, 200000, 1e-7, 100, False, 'CB'
    cls = scTelescope if sc else Telescope
    ts = cls.__new__(cls)
    ts.opts, ts.single_cell, ts.read_index, ts.feat_index, ts.shape, ts.raw_scores = Opts(), sc, {}, {}, None, None
    ts.run_info = OrderedDict([('version', VERSION)])
    ts.other_bam, ts.tmp_bam = os.path.join(outdir, 'other.bam'), os.path.join(outdir, 'tmp_tele.bam')
    if sc:
        ts.read_barcodes, ts.barcode_read_indices = {}, defaultdict(list)
    WRITTEN.clear()
    ts.load_alignment(GtfAnnotation(gtf))                     # _load_sequential -> the two BAMs, _mapping_to_matrix
    for p in (ts.other_bam, ts.tmp_bam):
        WRITTEN[p + '#refs'] = parse_bam(bam)[0]
    raw = ts.raw_scores.tocsr()
    np.random.seed(ts.get_random_seed())
    tl = TelescopeLikelihood(csr_matrix_plus(raw), Opts())
    tl.em(use_likelihood=False)
    ts.output_report(tl, os.path.join(outdir, 'stats.tsv'), os.path.join(outdir, 'counts.tsv'))
    seen = {}
    orig = tl.reassign

    def reassign(m, p=0.9, initial=False):                    # record the assignment update_sam draws (choose: a fresh draw)
        seen['mat'] = orig(m, p, initial)
        return seen['mat']
    tl.reassign = reassign
    ts.update_sam(tl, os.path.join(outdir, 'updated.bam'))
    rs = raw.copy(); rs.sort_indices()
    rows = np.repeat(np.arange(rs.shape[0]), np.diff(rs.indptr))
    z = np.asarray(tl.z.tocsr()[rows, rs.indices]).ravel().astype(np.float64)
    m = np.asarray(seen['mat'].tocsr()[rows, rs.indices]).ravel().astype(np.float64)
    txt = {k: [Seg(d, WRITTEN[ts.tmp_bam + '#refs']).text() for d in WRITTEN[os.path.join(outdir, k + '.bam')]]
           for k in ('other', 'tmp_tele', 'updated')}
    return txt, z, m, rs


def main():
    records = build_records()
    with open(os.path.join(GOLD, 'updated_mixed.bam'), 'wb') as f:
        f.write(L.bgzf(bam_bytes(records)))
    with open(os.path.join(GOLD, 'updated_mixed.gtf'), 'w') as f:
        f.write('# synthetic annotation for the --updated_sam tests (tools/make_updated_sam_fixture.py)\n')
        for chrom, s, e, strand, loc in GTF_ROWS:
            f.write('%s\tsynthetic\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; transcript_id "%s"; locus "%s";\n'
                    % (chrom, s, e, strand, loc, loc, loc))
    L.load_reference_loader()
    from telescope.utils import alignment
    alignment.AlignedPair = AlignedPair
    sys.modules['pysam'].AlignmentFile = AlignmentFile
    sys.modules['pysam'].FSECONDARY = 0x100
    cases = [('loader_mixed', False, False), ('sc_mixed', True, False), ('updated_mixed', False, False),
             ('bundled', False, True)]
    out_json, out_npz = OrderedDict(), {}
    for name, sc, big in cases:
        bam = os.path.join(GOLD, ('bundled_alignment' if name == 'bundled' else name) + '.bam')
        gtf = os.path.join(GOLD, ('bundled_annotation' if name == 'bundled' else name) + '.gtf')
        entry = OrderedDict()
        for mode in MODES:
            with tempfile.TemporaryDirectory() as d:
                txt, z, m, rs = reference_run(bam, gtf, mode, sc, d)
            if big:
                txt = {k: hashlib.sha256('\n'.join(v).encode()).hexdigest() for k, v in txt.items()}
            if mode == MODES[0]:
                entry['other'], entry['tmp_tele'] = txt['other'], txt['tmp_tele']
                out_npz['%s_indptr' % name], out_npz['%s_indices' % name] = rs.indptr.astype(np.int64), rs.indices.astype(np.int32)
            assert entry['other'] == txt['other'] and entry['tmp_tele'] == txt['tmp_tele']
            entry['updated_' + mode] = txt['updated']
            out_npz['%s_%s_z' % (name, mode)], out_npz['%s_%s_mask' % (name, mode)] = z, m
            print(name, mode, 'records', len(txt['updated']) if not big else txt['updated'][:16],
                  'z=0.125 entries', int(np.sum(z == 0.125)))
        out_json[name] = entry
    with open(os.path.join(GOLD, 'updated_sam_expected.json'), 'w') as f:
        json.dump(out_json, f, indent=0)
        f.write('\n')
    np.savez_compressed(os.path.join(GOLD, 'updated_sam_expected.npz'), **out_npz)


if __name__ == '__main__':
    main()
