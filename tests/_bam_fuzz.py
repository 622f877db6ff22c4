"""Seeded BAM + GTF cases for the device loader (no GPU needed): records are encoded with `struct` and written with
bam_out.BamWriter.  Every case holds, besides random bundles, one bundle (or a few) for each place where the kernels of
telescope_amd/csrc/tsem_bam.hip can go wrong; `Case.situations` counts them by name, SITUATIONS lists the names a case must have.

    case = make_case(seed, directory)      # -> Case(bam, gtf, situations, n_records, expected_fallbacks)

The loads of these cases use RECORD_CAP as `record_cap`: one bundle of every case is longer, and one pair hits 9 loci, so exactly
EXPECTED_FALLBACKS bundles go to the host.
"""
import os
import random
import struct
from collections import Counter, namedtuple

from telescope_amd.bam_out import BamWriter

RECORD_CAP = 64
EXPECTED_FALLBACKS = 2
OPS = 'MIDNSHP=X'
REFS = [('c1', 100000), ('c2', 50000), ('c3', 50000)]         # c3 is not in the GTF; the GTF's cX is not in the BAM
SITUATIONS = [
    'pair_duplicate_key', 'pair_missing_mate', 'pair_first_not_proper', 'pair_unmapped_PU', 'pair_mixed_unmapped_mate',
    'name_recurs', 'name_prefix',
    'cigar_N', 'cigar_D', 'cigar_I', 'cigar_S', 'cigar_H', 'cigar_P', 'cigar_=', 'cigar_X', 'cigar_zero_M', 'cigar_40_ops',
    'merge_interleaved', 'merge_overlapping', 'merge_dist_0', 'merge_dist_1', 'merge_dist_2',
    'block_end_touches_interval', 'two_loci_equal_overlap', 'two_exons_two_blocks',
    'threshold_rejected_10_of_50', 'threshold_accepted_11_of_50',
    'ref_not_in_gtf', 'gtf_chrom_not_in_bam',
    'AS_c', 'AS_C', 'AS_s', 'AS_S', 'AS_i', 'AS_I', 'AS_after_B', 'AS_after_Z', 'AS_after_H', 'AS_after_A', 'AS_after_f',
    'tie_score_plus_len_in_feature', 'tie_alnscore_across_features',
    'strand_forward_single', 'strand_reverse_single', 'strand_forward_pair', 'strand_reverse_pair', 'locus_minus_strand',
    'fallback_9_loci', 'fallback_over_record_cap',
]
GTF_ROWS = [                                                  # chrom, start, end (inclusive), strand, locus
    ('c1', 1000, 1999, '+', 'L_a'), ('c1', 1500, 2500, '-', 'L_over'), ('c1', 3000, 3499, '-', 'L_b'),
    ('c1', 5000, 5099, '+', 'L_2ex'), ('c1', 5300, 5399, '+', 'L_2ex'),
    ('c1', 8000, 8049, '+', 'L_t1'), ('c1', 8060, 8109, '+', 'L_t2'),
    ('c1', 12000, 12999, '+', 'L_p'), ('c1', 12000, 12499, '-', 'L_q'), ('c1', 30000, 39999, '+', 'L_big'),
    ('c2', 100, 9999, '+', 'L_c'), ('c2', 20000, 20999, '-', 'L_d'), ('cX', 10, 500, '+', 'L_x'),
] + [('c1', 20000 + 20 * k, 20009 + 20 * k, strand, 'L_%s%d' % (tag, k)) for k in range(9) for strand, tag in (('+', 'n'), ('-', 'm'))]
# (L_n* / L_m*: nine loci per strand within 200 bases, so that one read hits nine of them under every stranded mode)

Case = namedtuple('Case', 'bam gtf situations n_records expected_fallbacks')
_AS_FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I'}
_AS_RANGE = {'c': (-128, 127), 'C': (0, 255), 's': (-300, 300), 'S': (0, 600), 'i': (-1000, 1000), 'I': (0, 1000)}
_OTHER = {'B': b'XBBS' + struct.pack('<iHHH', 3, 1, 2, 3), 'Z': b'XZZhello\x00', 'H': b'XHH1AE3\x00', 'A': b'XAAq',
          'f': b'XFf' + struct.pack('<f', 1.5)}


def encode(name, flag, ref, pos, cigar, nref=-1, npos=-1, tlen=0, AS=None, as_type='c', before='', bc=None, umi=None):
    """One record's bytes (no block size).  cigar: [(length, op letter)]; AS None: no AS tag; `before`: letters of B Z H A f, the tags
    of those types that stand in front of AS."""
    l_seq = sum(n for n, op in cigar if op in 'MIS=X')
    body = struct.pack('<iiBBHHHiiii', ref, pos, len(name) + 1, 30, 0, len(cigar), flag, l_seq, nref, npos, tlen)
    body += name.encode() + b'\x00' + b''.join(struct.pack('<I', (n << 4) | OPS.index(op)) for n, op in cigar)
    body += bytes((l_seq + 1) // 2) + bytes([30]) * l_seq
    for t in before:
        body += _OTHER[t]
    if AS is not None:
        body += b'AS' + as_type.encode() + struct.pack(_AS_FMT[as_type], AS)
    if bc is not None:
        body += b'CBZ' + bc.encode() + b'\x00'
    if umi is not None:
        body += b'UBZ' + umi.encode() + b'\x00'
    body += b'NMC\x01'
    return body


class _Builder(object):
    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.bundles = []                                     # [[record bytes, ...], ...]
        self.sit = Counter()
        self.n = 0

    def name(self):
        self.n += 1
        return 'q%05d' % self.n

    def tags(self):
        r = self.rng
        return dict(bc=r.choice([None, 'AAAC', 'AAAG', 'CCTG']), umi=r.choice([None, 'TTA', 'GGC', 'ACA', 'TGT']))

    def single(self, name, ref, pos, cigar, AS=-3, rev=False, unmapped=False, **kw):
        flag = (0x10 if rev else 0) | (0x4 if unmapped else 0)
        return encode(name, flag, ref, pos, cigar, AS=AS, **kw)

    def pair(self, name, ref, pos1, cig1, pos2, cig2, AS1=-2, AS2=-4, rev=False, proper=True, tlen=None, **kw):
        """r1, r2 of one proper pair (read1 forward unless `rev`)"""
        t = (pos2 + 50 - pos1) if tlen is None else tlen
        f = 0x1 | (0x2 if proper else 0)
        r1 = encode(name, f | 0x40 | (0x10 if rev else 0x20), ref, pos1, cig1, ref, pos2, t, AS=AS1, **kw)
        r2 = encode(name, f | 0x80 | (0x20 if rev else 0x10), ref, pos2, cig2, ref, pos1, -t, AS=AS2, as_type=kw.get('as_type', 'c'))
        return [r1, r2]

    def add(self, records, *situations):
        self.bundles.append(records)
        for s in situations:
            self.sit[s] += 1

    def random_cigar(self, max_ops=8):
        r = self.rng
        ops = [(r.randint(5, 40), 'M')]
        for _ in range(r.randint(0, max_ops - 1)):
            op = r.choice('MIDNSP=XMM')
            ops.append((r.randint(0 if op == 'M' else 1, 60 if op == 'N' else 25), op))
        if r.random() < .3:
            ops = [(r.randint(1, 5), 'H')] + ops
        if r.random() < .3:
            ops.append((r.randint(1, 9), 'S'))
        return ops

    def count_cigar(self, cigar):
        for n, op in cigar:
            if op != 'M':
                self.sit['cigar_' + op] += 1
            elif n == 0:
                self.sit['cigar_zero_M'] += 1
        if len(cigar) >= 40:
            self.sit['cigar_40_ops'] += 1

    def random_pos(self):
        r = self.rng
        ref = r.choice([0, 0, 0, 1, 2])
        if ref == 0:
            pos = r.choice([r.randint(900, 2600), r.randint(2900, 3600), r.randint(4900, 5450), r.randint(7950, 8150),
                            r.randint(11900, 13100), r.randint(29900, 40100), r.randint(50000, 60000)])
        elif ref == 1:
            pos = r.choice([r.randint(0, 10100), r.randint(19900, 21100), r.randint(30000, 40000)])
        else:
            pos = r.randint(0, 40000)
        return ref, pos

    def random_bundle(self):
        r = self.rng
        name, recs = self.name(), []
        kind = r.random()
        as_type = r.choice('cCsSiI')
        val = lambda: r.randint(*_AS_RANGE[as_type])
        n_aln = r.choice([1, 1, 1, 2, 3, 5, 8])
        t = self.tags()
        if kind < .35:                                        # single-end
            for _ in range(n_aln):
                ref, pos = self.random_pos()
                cig = self.random_cigar(); self.count_cigar(cig)
                rev = r.random() < .5
                self.sit['strand_reverse_single' if rev else 'strand_forward_single'] += 1
                self.sit['AS_' + as_type] += 1
                recs.append(self.single(name, ref, pos, cig, AS=val(), rev=rev, as_type=as_type, **t))
            if r.random() < .1:
                recs.append(self.single(name, -1, -1, [], AS=None, unmapped=True))
        elif kind < .9:                                       # proper pairs, shuffled a little
            for _ in range(n_aln):
                ref, pos = self.random_pos()
                c1, c2 = self.random_cigar(), self.random_cigar()
                self.count_cigar(c1); self.count_cigar(c2)
                rev = r.random() < .5
                self.sit['strand_reverse_pair' if rev else 'strand_forward_pair'] += 1
                self.sit['AS_' + as_type] += 2
                recs += self.pair(name, ref, pos, c1, pos + r.randint(-30, 200), c2, val(), val(), rev=rev, as_type=as_type, **t)
            if r.random() < .3:
                r.shuffle(recs)
            if r.random() < .2 and len(recs) > 2:
                del recs[r.randrange(len(recs))]
                self.sit['pair_missing_mate'] += 1
        else:                                                 # improper pairs and unmapped mates
            for _ in range(n_aln):
                ref, pos = self.random_pos()
                cig = self.random_cigar(); self.count_cigar(cig)
                self.sit['AS_' + as_type] += 1
                recs.append(encode(name, 0x1 | 0x40 | 0x8, ref, pos, cig, ref, pos, 0, AS=val(), as_type=as_type, **t))
                recs.append(encode(name, 0x1 | 0x80 | 0x4, ref, pos, [], ref, pos, 0))
                self.sit['pair_mixed_unmapped_mate'] += 1
        self.bundles.append(recs)


def _special_bundles(b):
    """one bundle, or a few, per listed situation"""
    M = lambda n: [(n, 'M')]
    r = b.rng
    # ---- pairing
    n = b.name()
    p = b.pair(n, 0, 1100, M(50), 1300, M(50))
    b.add([p[0], p[0], p[1], b.pair(n, 0, 3100, M(50), 3200, M(50))[0], b.pair(n, 0, 3100, M(50), 3200, M(50), AS1=-9)[0]],
          'pair_duplicate_key', 'pair_duplicate_key', 'pair_missing_mate')       # equal keys with and without the mate arriving
    n = b.name()
    b.add(b.pair(n, 0, 1200, M(50), 1400, M(50)) + b.pair(n, 0, 5010, M(50), 5200, M(50))[:1], 'pair_missing_mate')
    n = b.name()
    b.add(b.pair(n, 0, 1250, M(50), 1450, M(50), proper=False)[:1] + b.pair(n, 0, 1250, M(50), 1450, M(50))
          + b.pair(n, 0, 3050, M(50), 3150, M(50)), 'pair_first_not_proper')
    n = b.name()
    b.add([encode(n, 0x1 | 0x4 | 0x8 | 0x40, -1, -1, []), encode(n, 0x1 | 0x4 | 0x8 | 0x80, -1, -1, [])], 'pair_unmapped_PU')
    n = b.name()
    b.add([encode(n, 0x1 | 0x8 | 0x40, 0, 1300, M(60), 0, 1300, 0, AS=-1), encode(n, 0x1 | 0x4 | 0x80, 0, 1300, [], 0, 1300, 0),
           encode(n, 0x1 | 0x8 | 0x40 | 0x100, 0, 3100, M(60), 0, 3100, 0, AS=-6)], 'pair_mixed_unmapped_mate')
    # ---- names
    b.add([b.single('rec1', 0, 1100, M(50), AS=-2, bc='AAAC', umi='TTA')], 'name_recurs')
    b.add([b.single('f1', 0, 1150, M(50), AS=-2), b.single('f10', 0, 1160, M(50), AS=-2), b.single('f10', 0, 3100, M(50), AS=-7),
           b.single('f100', 0, 1170, M(50), AS=-2)], 'name_prefix', 'name_prefix')           # three bundles in a row: f1, f10 x 2, f100
    b.add([b.single('f1', 0, 3160, M(50), AS=-2)], 'name_recurs')
    b.add([b.single('rec1', 0, 3100, M(50), AS=-1, bc='CCTG', umi='GGC')])
    # ---- CIGARs
    cig = [(10, 'M'), (0, 'M'), (3, 'I'), (5, 'M'), (2, 'D'), (8, '='), (1, 'X'), (30, 'N'), (6, 'M'), (1, 'P'), (4, 'M')]
    full = [(2, 'H'), (3, 'S')] + cig + [(4, 'S'), (1, 'H')]
    b.count_cigar(full)
    b.add([b.single(b.name(), 0, 1010, full)])
    long_cig = []
    for k in range(20):
        long_cig += [(r.randint(1, 9), 'M'), (r.randint(1, 3), r.choice('DNI'))]
    b.count_cigar(long_cig)
    b.add([b.single(b.name(), 0, 30100, long_cig)])
    # ---- block merging: r1 blocks [p, p+20) and [p+60, p+80); r2 fills in at a distance d behind r1's first block
    for d, tag in ((0, 'merge_dist_0'), (1, 'merge_dist_1'), (2, 'merge_dist_2')):
        b.add(b.pair(b.name(), 0, 31000, [(20, 'M'), (40, 'N'), (20, 'M')], 31020 + d, M(15)), tag, 'merge_interleaved')
    b.add(b.pair(b.name(), 0, 32000, M(50), 32030, M(50)), 'merge_overlapping')
    b.add(b.pair(b.name(), 0, 32030, M(50), 32000, [(10, 'M'), (25, 'N'), (40, 'M')]), 'merge_overlapping', 'merge_interleaved')
    # ---- intersection
    b.add([b.single(b.name(), 0, 2950, M(50), AS=-1)], 'block_end_touches_interval')         # [2950, 3000): the query ends at 3001
    b.add([b.single(b.name(), 0, 8030, M(50), AS=-1)], 'two_loci_equal_overlap')             # 20 in L_t1, 20 in L_t2 (+1 at the end)
    b.add([b.single(b.name(), 0, 8029, M(51), AS=-1)], 'two_loci_equal_overlap')             # 21 and 21: the first inserted wins
    b.add([b.single(b.name(), 0, 5080, [(20, 'M'), (200, 'N'), (20, 'M')], AS=-1)], 'two_exons_two_blocks')
    # ---- threshold: alnlen 50 against L_a = [1000, 2000); a block [s, s + 50) asks for [s, s + 51)
    b.add([b.single(b.name(), 0, 959, M(50), AS=-1)], 'threshold_rejected_10_of_50')
    b.add([b.single(b.name(), 0, 960, M(50), AS=-1)], 'threshold_accepted_11_of_50')
    # ---- references
    b.add([b.single('onc3', 2, 1000, M(50)), b.single('onc3', 0, 1100, M(50), AS=-8)], 'ref_not_in_gtf')
    b.sit['gtf_chrom_not_in_bam'] += 1
    # ---- aux fields
    for t in 'cCsSiI':
        lo, hi = _AS_RANGE[t]
        b.add([b.single('as_' + t, 0, 1100, M(50), AS=hi, as_type=t), b.single('as_' + t, 0, 3100, M(50), AS=lo, as_type=t)], 'AS_' + t)
    for t in 'BZHAf':
        b.add([b.single('aux_' + t, 0, 1100, M(50), AS=-4, before=t + 'ZB')], 'AS_after_' + t)
    # ---- ordering ties
    n = b.name()
    b.add([b.single(n, 0, 1100, M(50), AS=10), b.single(n, 0, 1700, M(48), AS=12, rev=True), b.single(n, 0, 3100, M(50), AS=10)],
          'tie_score_plus_len_in_feature', 'tie_alnscore_across_features')
    n = b.name()
    b.add([b.single(n, 0, 3100, M(50), AS=7), b.single(n, 1, 200, M(50), AS=9), b.single(n, 0, 1100, M(50), AS=7),
           b.single(n, 0, 5010, M(50), AS=9)], 'tie_alnscore_across_features')
    # ---- strands
    b.add([b.single(b.name(), 0, 12100, M(50), rev=False)], 'strand_forward_single', 'locus_minus_strand')
    b.add([b.single(b.name(), 0, 12100, M(50), rev=True)], 'strand_reverse_single', 'locus_minus_strand')
    b.add(b.pair(b.name(), 0, 12100, M(50), 12300, M(50), rev=False), 'strand_forward_pair', 'locus_minus_strand')
    b.add(b.pair(b.name(), 0, 12100, M(50), 12300, M(50), rev=True), 'strand_reverse_pair', 'locus_minus_strand')
    # ---- fallbacks
    b.add([b.single(b.name(), 0, 19995, M(200), AS=-3)], 'fallback_9_loci')
    n = b.name()
    big = []
    for k in range(RECORD_CAP // 2 + 2):
        big += b.pair(n, 0, 1000 + 13 * k, M(50), 1200 + 13 * k, M(50), AS1=-k, AS2=-1)
    b.add(big, 'fallback_over_record_cap')


def make_case(seed, directory):
    b = _Builder(seed)
    _special_bundles(b)
    n_special = len(b.bundles)
    target = b.rng.randint(260, 1200)
    while sum(len(x) for x in b.bundles) < target:
        b.random_bundle()
    # the special bundles keep their order (names recur on purpose) and are spread between the random ones
    special, rest = b.bundles[:n_special], b.bundles[n_special:]
    slots = sorted(b.rng.sample(range(len(rest) + 1), min(n_special, len(rest) + 1)))
    while len(slots) < n_special:
        slots.append(len(rest))
    order, k = [], 0
    for i in range(len(rest) + 1):
        while k < n_special and slots[k] == i:
            order.append(special[k]); k += 1
        if i < len(rest):
            order.append(rest[i])
    bam = os.path.join(directory, 'fuzz_%d.bam' % seed)
    gtf = os.path.join(directory, 'fuzz_%d.gtf' % seed)
    refs_block = struct.pack('<i', len(REFS)) + b''.join(
        struct.pack('<i', len(n) + 1) + n.encode() + b'\x00' + struct.pack('<i', l) for n, l in REFS)
    text = '@HD\tVN:1.6\tSO:unsorted\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % x for x in REFS)
    with BamWriter(bam, dict(text=text, refs_block=refs_block)) as w:
        for bundle in order:
            for rec in bundle:
                w.write(rec)
    with open(gtf, 'w') as fh:
        fh.write('# fuzz case %d\n' % seed)
        for chrom, s, e, strand, loc in GTF_ROWS:
            fh.write('%s\tfuzz\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; locus "%s";\n' % (chrom, s, e, strand, loc, loc))
    return Case(bam, gtf, b.sit, sum(len(x) for x in order), EXPECTED_FALLBACKS)
