#!/usr/bin/env python3
"""Single-cell fixture: a small synthetic BAM with cell barcodes (CB tags) + GTF, and what the REFERENCE derives from it.

DEV-CONTAINER ONLY (imports /root/reference through tools/make_loader_fixture.py and tools/ref_import.py).  Writes
    tests/golden/sc_mixed.bam / sc_mixed.gtf     the loader fixture's fragment classes with CB tags, plus fragments without a tag, a tag
                                                 only on read 2, barcodes whose fragments all miss the annotation, unmapped fragments
                                                 with a barcode, interleaved barcodes (first appearance != sorted order) and enough
                                                 fragments per cell for exclude / choose / average to differ
    tests/golden/sc_expected.npz                 per stranded mode: the matrix, cell_of_row and the barcodes — the reference's own
                                                 barcode capture (model.py:245-247, restated with pysam's names `has_tag` / `get_tags`
                                                 like the loop around it, tools/make_loader_fixture.py) and `_mapping_to_matrix`
                                                 (model.py:287-362, incl. barcode_read_indices, 311-316) run unmodified
    tests/golden/sc_ref-run_stats.tsv, sc_ref-TE_counts_<method>.tsv
                                                 written by the reference's own `scTelescope.output_report` (model.py:575-629) after
                                                 its own TelescopeLikelihood.em(), with use_every_reassign_mode and the run's seed
                                                 (telescope_assign.py:428-440); run_info holds the counters `sc assign` writes
"""
import os
import struct
import sys
from collections import Counter, OrderedDict, defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import make_loader_fixture as L  # noqa: E402

GOLD = L.GOLD
TAG = 'CB'
VERSION = '1.0.3.1-mi355x'
GTF_ROWS = L.GTF_ROWS + [('chrB', 10000, 10999, '+', 'L6'), ('chrB', 20000, 20999, '+', 'L7')]   # two loci of equal support (ties)


def build_records():
    """The loader fixture's records with barcodes, plus single-cell cases."""
    R = L.build_records()
    bc = {'f01': 'TTTG', 'f02': 'AAAC', 'f04': 'TTTG', 'f05': 'CCCA', 'f06': 'AAAC', 'f08': 'GGGT', 'f09': 'CCCA',
          'f10': 'NOFEAT', 'f11': 'TTTG', 'f12': 'NOFEAT', 'f13': 'AAAC', 'f14': 'GGGT', 'f15': 'TTTG', 'f16': 'CCCA',
          'f17': 'GGGT', 'f18': 'AAAC', 'f03': 'UNMAPPED', 'f07': 'UNMAPPED'}
    for r in R:
        if r['qname'] in bc and not (r['flag'] & L.R2):
            r['CB'] = bc[r['qname']]
    # f09: read 2 tagged too (a PX pair): r1 decides
    # more fragments: ambiguous reads in three cells so that exclude / choose / average / conf differ, interleaved barcodes
    cells = ['TTTG', 'AAAC', 'CCCA', 'GGGT', 'ACGT']
    rng = np.random.RandomState(17)
    hits = [(0, 1100), (0, 1250), (0, 5100), (0, 5300), (0, 9200), (0, 9500), (1, 200), (1, 600), (0, 1700)]
    for i in range(60):
        q = 'g%02d' % i
        n = 1 + rng.randint(0, 3)
        pick = rng.choice(len(hits), n, replace=False)
        AS = -int(rng.randint(0, 4))
        recs = []
        for j, h in enumerate(pick):
            ref, pos = hits[h]
            recs.append(L.rec(q, 0 if j == 0 else L.SECONDARY, ref, pos + int(rng.randint(0, 40)), '50M',
                              AS if rng.rand() < 0.6 else AS - int(rng.randint(1, 5))))
        if i % 11 == 3:
            pass                                          # no tag at all
        elif i % 11 == 7:
            R += L.pair(q, 0, 1300 + i, '50M', -2, 1500 + i, '50M', -2, 250)
            R[-1]['CB'] = 'R2ONLY'                        # a tag on read 2 only: does not count
            continue
        else:
            recs[0]['CB'] = cells[(i * 7) % len(cells)]
        R += recs
    # two loci with the same support (L6, L7: same length, the same unique fragments): fragments that hit both with the same score
    # and length keep EXACTLY tied posteriors through EM, so `exclude` drops them, `choose` draws one locus, `average` splits them
    for i in range(4):
        for ref_pos, loc in ((10100, 'L6'), (20100, 'L7')):
            R += [L.rec('u%s_%d' % (loc, i), 0, 1, ref_pos + 37 * i, '50M', -2)]
            R[-1]['CB'] = cells[i % len(cells)]
    for i in range(9):
        q = 't%02d' % i
        R += [L.rec(q, 0, 1, 10300 + 11 * i, '50M', -1), L.rec(q, L.SECONDARY, 1, 20300 + 11 * i, '50M', -1)]
        R[-2]['CB'] = cells[(3 * i) % len(cells)]
    R += [L.rec('h01', L.UNMAP)]
    R[-1]['CB'] = 'UNMAPPED'                              # an unmapped fragment with a barcode
    R += [L.rec('h02', 0, 0, 60000, '50M', -1)]
    R[-1]['CB'] = 'NOFEAT'                                # all of this barcode's fragments miss the annotation
    return R


def bam_bytes(records):
    """tools/make_loader_fixture.py's encoder, plus the CB tag (Z) where a record has one."""
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
        body = struct.pack('<iiBBHHHiiii', r['ref_id'], r['pos'], len(qn), 30, 4680, len(cig), r['flag'], l_seq,
                           r['nref'], r['npos'], r['tlen'])
        body += qn + b''.join(struct.pack('<I', (n << 4) | o) for n, o in cig)
        body += bytes([0x11] * ((l_seq + 1) // 2)) + bytes([30] * l_seq)
        body += b'NMC\x00'
        if r['AS'] is not None:
            body += b'ASi' + struct.pack('<i', r['AS'])
        body += b'XSZ' + b'note\x00'
        if r.get('CB'):
            body += b'CBZ' + r['CB'].encode() + b'\x00'
        body += b'UBZ' + b'UMI1\x00'                      # another Z tag after the barcode
        out += struct.pack('<i', len(body)) + body
    return bytes(out)


class Seg(L.Seg):
    def __init__(self, r):
        super().__init__(r)
        if r.get('CB'):
            self._tags['CB'] = r['CB']

    def has_tag(self, t):
        return t in self._tags or (t == 'AS' and self._AS is not None)

    def get_tags(self):
        return list(self._tags.items()) + ([('AS', self._AS)] if self._AS is not None else [])


class SamStub(L.SamStub):
    def fetch(self, **kw):
        return iter([Seg(r) for r in self.records])


def expected(records, stranded_mode, Telescope, alignment, model, threshold=0.2):
    """tools/make_loader_fixture.expected plus the reference's barcode capture and barcode_read_indices."""
    annot = L.BruteAnnotation(GTF_ROWS, stranded_mode)

    def assign(pair):
        if pair.r1_is_reversed:
            strand = ('+' if stranded_mode[-1] == 'F' else '-') if pair.is_paired else ('-' if stranded_mode[0] == 'F' else '+')
        else:
            strand = ('-' if stranded_mode[-1] == 'F' else '+') if pair.is_paired else ('+' if stranded_mode[0] == 'F' else '-')
        f = annot.intersect_blocks(pair.ref_name, pair.refblocks, strand)
        if not f:
            return L.NOFEAT
        fname, overlap = f.most_common()[0]
        return fname if overlap > pair.alnlen * threshold else L.NOFEAT

    info, mappings, read_barcodes = Counter(), [], {}
    min_as, max_as = 2 ** 32 - 1, -(2 ** 32 - 1)
    for ci, alns in alignment.fetch_fragments_seq(SamStub(records), until_eof=True):
        info['total_fragments'] += 1
        code = alignment.CODES[ci][0]
        info[code] += 1
        if code in ('SU', 'PU'):
            continue
        if alns[0].r1.has_tag(TAG):                                                   # model.py:245-247
            read_barcodes[alns[0].query_id] = dict(alns[0].r1.get_tags()).get(TAG)
        mapped = [a for a in alns if not a.is_unmapped]
        ambig = len(mapped) > 1
        scores = [a.alnscore for a in mapped]
        min_as, max_as = min(min_as, *scores), max(max_as, *scores)
        feats = list(map(assign, mapped))
        if not any(f != L.NOFEAT for f in feats):
            info['nofeat_%s' % ('A' if ambig else 'U')] += 1
            continue
        info['feat_%s' % ('A' if ambig else 'U')] += 1
        for m in model.process_overlap_frag(mapped, feats):
            mappings.append((ci, m[0], m[1], m[2], m[3]))

    class O(object):
        no_feature_key = L.NOFEAT
    ts = Telescope.__new__(Telescope)
    ts.opts, ts.single_cell, ts.read_index, ts.feat_index, ts.run_info = O(), True, {}, {}, {}
    ts.read_barcodes, ts.barcode_read_indices = read_barcodes, defaultdict(list)
    Telescope._mapping_to_matrix(ts, iter(mappings), (min_as, max_as), info)          # the reference's own, barcodes included
    raw = ts.raw_scores.tocsr()
    raw.sort_indices()
    cor = np.full(raw.shape[0], -1, np.int32)
    barcodes = [b for b, rows in ts.barcode_read_indices.items() if len(rows) > 0]     # model.py:616-617
    for c, b in enumerate(barcodes):
        cor[ts.barcode_read_indices[b]] = c
    return ts, annot, info, dict(data=raw.data.astype(np.uint16), indices=raw.indices.astype(np.int32),
                                 indptr=raw.indptr.astype(np.int64), shape=np.array(raw.shape), cell_of_row=cor,
                                 barcodes=np.array(barcodes, dtype=np.str_))


def reference_reports(ts, annot, info, exp):
    """The reference's own EM and scTelescope.output_report with every reassign mode, seeded like telescope_assign.py:428-431."""
    import scipy.sparse as sp
    from telescope.utils.model import TelescopeLikelihood, scTelescope
    from telescope.utils.sparse_plus import csr_matrix_plus

    class Opts(object):
        reassign_mode, conf_prob, use_every_reassign_mode = 'exclude', 0.9, True
        pi_prior, theta_prior, em_epsilon, max_iter, use_likelihood = 0, 200000, 1e-7, 100, False
    # run_info: what `sc assign` writes — version, annotated features, then the loader's counters (tests/test_loader_mixed.py holds
    # those equal to the reference's own)
    from telescope_amd import loader
    r = loader.load_alignment(os.path.join(GOLD, 'sc_mixed.bam'), loader.Annotation(os.path.join(GOLD, 'sc_mixed.gtf')))
    raw = sp.csr_matrix((exp['data'], exp['indices'], exp['indptr']), shape=tuple(exp['shape']))
    sc = scTelescope.__new__(scTelescope)
    sc.opts = Opts()
    sc.run_info = OrderedDict([('version', VERSION), ('annotated_features', len(set(g[4] for g in GTF_ROWS)))] +
                              list(r['run_info'].items()))
    sc.feat_index = ts.feat_index
    fl = annot.feature_length()
    sc.feature_length = Counter({f: fl[f] for f in ts.feat_index})
    sc.barcode_read_indices = ts.barcode_read_indices
    shape = raw.shape
    seed = (sc.run_info['total_fragments'] % shape[0] * shape[1]) % 4294967295     # model.py:150-153
    np.random.seed(seed)
    tl = TelescopeLikelihood(csr_matrix_plus(raw), Opts())
    tl.em(use_likelihood=False)
    sc.output_report(tl, os.path.join(GOLD, 'sc_ref-run_stats.tsv'), os.path.join(GOLD, 'sc_ref-TE_counts.tsv'))


def main():
    records = build_records()
    with open(os.path.join(GOLD, 'sc_mixed.bam'), 'wb') as f:
        f.write(L.bgzf(bam_bytes(records)))
    with open(os.path.join(GOLD, 'sc_mixed.gtf'), 'w') as f:
        f.write('# synthetic annotation for tests/test_sc_host.py and tests/test_gpu_sc.py (tools/make_sc_fixture.py)\n')
        for chrom, s, e, strand, loc in GTF_ROWS:
            f.write('%s\tsynthetic\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; transcript_id "%s"; locus "%s";\n'
                    % (chrom, s, e, strand, loc, loc, loc))
    Telescope, alignment, model = L.load_reference_loader()
    out = {}
    for mode in ('None', 'F', 'R', 'FR', 'RF'):
        ts, annot, info, e = expected(records, mode, Telescope, alignment, model)
        for k, v in e.items():
            out['%s_%s' % (mode, k)] = v
        print(mode, 'matrix %s' % (tuple(e['shape']),), 'cells', list(e['barcodes']))
        if mode == 'None':
            reference_reports(ts, annot, info, e)
    np.savez_compressed(os.path.join(GOLD, 'sc_expected.npz'), **out)


if __name__ == '__main__':
    main()
