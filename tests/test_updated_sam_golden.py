"""`--updated_sam` against what the REFERENCE writes (tests/golden/updated_sam_expected.*, tools/make_updated_sam_fixture.py: the
reference's own _load_sequential and update_sam on pysam-named stubs).  No GPU: the record rewrite is fed the reference's own z and
assignment at every stored entry, as tag words."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLD

MODES = ('exclude', 'choose', 'average', 'conf', 'unique')
CASES = {'loader_mixed': False, 'sc_mixed': True, 'updated_mixed': False, 'bundled': False}


def expected():
    with open(os.path.join(GOLD, 'updated_sam_expected.json')) as f:
        return json.load(f)


def inputs(name):
    stem = 'bundled_alignment' if name == 'bundled' else name
    gtf = 'bundled_annotation' if name == 'bundled' else name
    return os.path.join(GOLD, stem + '.bam'), os.path.join(GOLD, gtf + '.gtf')


def texts(path):
    from telescope_amd import bam_out, loader
    _, recs, header = loader.read_bam(path, raw=True)
    return [bam_out.record_text(s.raw) for s in recs], header


def same(got, want):
    """canonical record text, or its SHA-256 (the bundled BAM)"""
    if isinstance(want, str):
        return hashlib.sha256('\n'.join(got).encode()).hexdigest() == want
    return got == want


class Opts(object):
    def __init__(self, samfile, gtffile, outdir, mode):
        self.samfile, self.gtffile, self.outdir, self.exp_tag = samfile, gtffile, outdir, 'telescope'
        self.attribute, self.no_feature_key, self.overlap_mode, self.overlap_threshold = 'locus', '__no_feature', 'threshold', 0.2
        self.stranded_mode, self.reassign_mode, self.conf_prob, self.updated_sam = 'None', mode, 0.9, True
        self.barcode_tag, self.version = 'CB', 'test'

    def outfile_path(self, suffix):
        return os.path.join(self.outdir, '%s-%s' % (self.exp_tag, suffix))


class StoredModel(object):
    """what update_sam asks of the likelihood, answered from the reference's stored z / assignment (tag words on the host)"""
    comm = None

    def __init__(self, words, indptr):
        self.words, self.indptr = words, indptr

    def reassign(self, method, thresh=0.9, initial=False):
        return None

    def entry_tag_tiles(self, method, thresh=0.9, assignment=None):
        n = len(self.indptr) - 1
        for r0 in range(0, n, 7):                                  # tiles of 7 rows
            r1 = min(n, r0 + 7)
            yield r0, r1, self.words[self.indptr[r0]:self.indptr[r1]]

    def entry_tags(self, r0, r1, method='exclude', thresh=0.9, assignment=None):
        return self.words[self.indptr[r0]:self.indptr[r1]]


@pytest.mark.parametrize('name', list(CASES))
def test_load_writes_the_references_other_and_tmp_bams(tmp_path, name):
    from telescope_amd import loader
    from telescope_amd.run_container import Telescope, scTelescope
    exp = expected()[name]
    bam, gtf = inputs(name)
    o = Opts(bam, gtf, str(tmp_path), 'exclude')
    ts = scTelescope(o) if CASES[name] else Telescope(o)
    ts.load_alignment(loader.Annotation(gtf))
    inp, header = texts(bam)
    for key, path in (('other', ts.other_bam), ('tmp_tele', ts.tmp_bam)):
        got, h = texts(path)
        assert h == header
        assert same(got, exp[key]), (name, key)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(CASES))
def test_rewrite_with_the_references_z_reproduces_its_records(tmp_path, name, mode):
    """Telescope.update_sam's host side, fed tag words made from the reference's own z and `mat` at every stored entry: the
    reference's updated records exactly (set_tag replacement of ZB / XP / YC, record order, unmapped mates, SEC pairs)."""
    from telescope_amd import bam_out, loader
    from telescope_amd.run_container import Telescope, scTelescope
    exp = expected()[name]
    f = np.load(os.path.join(GOLD, 'updated_sam_expected.npz'))
    bam, gtf = inputs(name)
    o = Opts(bam, gtf, str(tmp_path), mode)
    ts = scTelescope(o) if CASES[name] else Telescope(o)
    ts.load_alignment(loader.Annotation(gtf))
    raw = ts.raw_scores
    assert np.array_equal(raw.indptr, f['%s_indptr' % name]) and np.array_equal(raw.indices, f['%s_indices' % name])
    words = bam_out.tag_word(f['%s_%s_z' % (name, mode)], f['%s_%s_mask' % (name, mode)])
    ts.update_sam(StoredModel(words, raw.indptr), o.outfile_path('updated.bam'), command_line='telescope assign test')
    got, h = texts(o.outfile_path('updated.bam'))
    assert same(got, exp['updated_' + mode]), (name, mode)
    _, hin = texts(bam)
    assert h['text'] == bam_out.header_with_pg(hin['text'], 'test', 'telescope assign test')


def test_the_small_fixture_covers_what_it_is_for():
    """updated_mixed: an XP rounding tie (z = 0.125 -> XP 12), old XP / YC replaced (moved to the end) on PRI, XP kept on SEC,
    an unmapped PX mate written unchanged with its old tags, exact 8-way ties"""
    exp = expected()['updated_mixed']['updated_exclude']
    h = [t for t in exp if t.startswith('h00\t')]
    assert len(h) == 8 and all('XP:C:12\t' in t for t in h)
    u03 = [t for t in exp if t.startswith('u03\t')][0]
    assert u03.endswith('XP:C:100\tYC:Z:217,95,2') and 'XP:Z:old' not in u03
    assert any(t.startswith('k01\t') and 'XP:Z:old' in t and t.endswith('YC:Z:248,248,248') for t in exp)
    assert 'p01\t133\t30\tXP:Z:old\tYC:Z:0,0,0' in exp
