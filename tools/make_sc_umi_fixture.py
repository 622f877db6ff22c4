#!/usr/bin/env python3
"""UMI fixture: a small synthetic BAM with cell barcodes (CB) and UMIs (UB) + GTF, and what the project's own definition makes of it.

The reference project has no UMI handling, so nothing here comes from it: the records are this file's own, the matrix is the one
telescope_amd/loader.py builds (held to the reference's loader by tests/test_loader_mixed.py and tests/test_sc_host.py on their
fixtures) and the representatives are those of the plain host definition, tests/_umi_reference.py.  Writes
    tests/golden/sc_umi.bam / sc_umi.gtf   single-end fragments of four cells over eight loci: several UMIs per cell; a chain of three
                                           fragments (A-B, B-C share a locus, A and C do not); a class that splits into two
                                           components; a score tie inside a component; one UMI shared by two cells; fragments
                                           without UB, without CB and without both; unmapped and unannotated fragments with tags
    tests/golden/sc_umi_expected.npz       the matrix, cell_of_row / barcodes, umi_of_row / umis, rep_of_row and stats
"""
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from tools import make_loader_fixture as L  # noqa: E402  (rec(), bgzf(), REFS, OPS: the BAM encoder's pieces)

GOLD = L.GOLD
LOCI = ['U%d' % i for i in range(1, 9)]
GTF_ROWS = [('chrA', 1000 + 5000 * i, 1999 + 5000 * i, '+', name) for i, name in enumerate(LOCI)]
CELLS = ['GATTACA', 'CCGGTTA', 'TTAGGCA', 'ACACGTG']


def frag(q, hits, cb=None, ub=None):
    """one single-end fragment: hits = [(locus number 1..8, offset, AS), ...], the first one primary"""
    out = []
    for j, (loc, off, AS) in enumerate(hits):
        out.append(L.rec(q, 0 if j == 0 else L.SECONDARY, 0, GTF_ROWS[loc - 1][1] + off, '50M', AS))
    if cb:
        out[0]['CB'] = cb
    if ub:
        out[0]['UB'] = ub
    return out


def build_records():
    R = []
    c0, c1, c2, c3 = CELLS
    # a chain of three: A-B share U2, B-C share U3, A and C share nothing; B has the best score
    R += frag('chainA', [(1, 10, -3), (2, 10, -3)], c0, 'CHAIN')
    R += frag('chainB', [(2, 30, -1), (3, 30, -2)], c0, 'CHAIN')
    R += frag('chainC', [(3, 50, -3), (4, 50, -3)], c0, 'CHAIN')
    # one class, two components: two fragments on U1, two on U5
    R += frag('splitA', [(1, 100, -2)], c0, 'SPLIT')
    R += frag('splitB', [(5, 100, -1)], c0, 'SPLIT')
    R += frag('splitC', [(1, 120, -1)], c0, 'SPLIT')
    R += frag('splitD', [(5, 120, -4)], c0, 'SPLIT')
    # a score tie inside a component: the first fragment stays
    R += frag('tieA', [(2, 200, -2)], c1, 'TIE')
    R += frag('tieB', [(2, 220, -2), (6, 220, -4)], c1, 'TIE')
    R += frag('tieC', [(6, 240, -2)], c1, 'TIE')
    # one UMI in two cells: never merged across the cells
    R += frag('shareA', [(3, 300, -1)], c0, 'SHARE')
    R += frag('shareB', [(3, 310, -2)], c1, 'SHARE')
    R += frag('shareC', [(3, 320, -2)], c0, 'SHARE')
    R += frag('shareD', [(3, 330, -1)], c1, 'SHARE')
    # tags missing
    R += frag('noUB1', [(4, 400, -1)], c2, None)
    R += frag('noUB2', [(4, 410, -1)], c2, None)
    R += frag('noCB1', [(4, 420, -1)], None, 'LONE')
    R += frag('noCB2', [(4, 430, -1)], None, 'LONE')
    R += frag('none1', [(4, 440, -1)], None, None)
    # a UMI on read records that never become rows
    R += [L.rec('unmapped1', L.UNMAP)]
    R[-1]['CB'], R[-1]['UB'] = c3, 'GHOST'
    R += [L.rec('nofeat1', 0, 1, 40000, '50M', -1)]
    R[-1]['CB'], R[-1]['UB'] = c3, 'GHOST'
    # the bulk: four cells, six UMIs each, one to three of the eight loci per fragment
    rng = np.random.RandomState(23)
    for i in range(170):
        cell = CELLS[(i * 3) % 4]
        umi = 'M%d%s' % (rng.randint(0, 6), cell[:2])
        n = 1 + int(rng.randint(0, 3))
        loci = 1 + rng.choice(8, n, replace=False)
        AS = -int(rng.randint(0, 4))
        hits = [(int(loc), int(rng.randint(0, 900)), AS if j == 0 or rng.rand() < 0.5 else AS - int(rng.randint(1, 4)))
                for j, loc in enumerate(loci)]
        R += frag('b%03d' % i, hits, cell, umi)
    return R


def bam_bytes(records):
    """single-end records with NM, AS and, where a record has them, CB and UB (both Z)"""
    out = bytearray(b'BAM\x01')
    text = '@HD\tVN:1.6\tSO:unsorted\tGO:query\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % r for r in L.REFS)
    out += struct.pack('<i', len(text)) + text.encode()
    out += struct.pack('<i', len(L.REFS))
    for name, ln in L.REFS:
        out += struct.pack('<i', len(name) + 1) + name.encode() + b'\x00' + struct.pack('<i', ln)
    for r in records:
        cig = [(int(n), L.OPS[o]) for n, o in L.re.findall(r'(\d+)([MIDNSHP=X])', r['cigar'])]
        l_seq = sum(n for n, o in cig if o in (0, 1, 4, 7, 8)) or 30
        qn = r['qname'].encode() + b'\x00'
        body = struct.pack('<iiBBHHHiiii', r['ref_id'], r['pos'], len(qn), 30, 4680, len(cig), r['flag'], l_seq, r['nref'], r['npos'], r['tlen'])
        body += qn + b''.join(struct.pack('<I', (n << 4) | o) for n, o in cig)
        body += bytes([0x11] * ((l_seq + 1) // 2)) + bytes([30] * l_seq)
        body += b'NMC\x00'
        if r['AS'] is not None:
            body += b'ASi' + struct.pack('<i', r['AS'])
        if r.get('UB'):
            body += b'UBZ' + r['UB'].encode() + b'\x00'      # (before the barcode here, behind it in sc_mixed.bam)
        if r.get('CB'):
            body += b'CBZ' + r['CB'].encode() + b'\x00'
        out += struct.pack('<i', len(body)) + body
    return bytes(out)


def main():
    from _umi_reference import dedup_plain
    from telescope_amd import loader
    records = build_records()
    bam, gtf = os.path.join(GOLD, 'sc_umi.bam'), os.path.join(GOLD, 'sc_umi.gtf')
    with open(bam, 'wb') as f:
        f.write(L.bgzf(bam_bytes(records)))
    with open(gtf, 'w') as f:
        f.write('# synthetic annotation for tests/test_umi_host.py and tests/test_gpu_umi_dedup.py (tools/make_sc_umi_fixture.py)\n')
        for chrom, s, e, strand, loc in GTF_ROWS:
            f.write('%s\tsynthetic\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; transcript_id "%s"; locus "%s";\n' % (chrom, s, e, strand, loc, loc, loc))
    r = loader.load_alignment(bam, loader.Annotation(gtf), barcode_tag='CB', umi_tag='UB')
    raw = r['raw_scores'].tocsr()
    cor, uor = r['cell_of_row'], r['umi_of_row']
    rep, stats = dedup_plain(raw.indptr, raw.indices, raw.data, cor, uor)
    row = r['read_index']
    # the fixture holds what it is meant to hold
    assert rep[row['chainA']] == rep[row['chainC']] == row['chainB']
    assert rep[row['splitA']] == rep[row['splitC']] == row['splitC'] and rep[row['splitB']] == rep[row['splitD']] == row['splitB']
    assert rep[row['tieA']] == rep[row['tieB']] == rep[row['tieC']] == row['tieA']
    assert rep[row['shareA']] == rep[row['shareC']] == row['shareA'] and rep[row['shareB']] == rep[row['shareD']] == row['shareD']
    assert uor[row['shareA']] == uor[row['shareB']] and cor[row['shareA']] != cor[row['shareB']]
    assert uor[row['noUB1']] == -1 and cor[row['noUB1']] >= 0 and cor[row['noCB1']] == -1 and uor[row['noCB1']] >= 0
    assert cor[row['none1']] == -1 and uor[row['none1']] == -1 and 'GHOST' not in r['umis']
    assert all(len(set(uor[(cor == c) & (uor >= 0)])) >= 4 for c in range(4))
    np.savez_compressed(os.path.join(GOLD, 'sc_umi_expected.npz'), data=raw.data.astype(np.uint16), indices=raw.indices.astype(np.int32),
                        indptr=raw.indptr.astype(np.int64), shape=np.array(raw.shape), cell_of_row=cor, barcodes=np.array(r['barcodes'], dtype=np.str_),
                        umi_of_row=uor, umis=np.array(r['umis'], dtype=np.str_), rep_of_row=rep, stats=stats)
    print('matrix %s, %d records, cells %s, %d UMIs, stats %s (rows in classes, classes, components, dropped)'
          % (raw.shape, len(records), r['barcodes'], len(r['umis']), stats.tolist()))


if __name__ == '__main__':
    main()
