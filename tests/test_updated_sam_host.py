"""`--updated_sam` on the host (no GPU): the BGZF / BAM writer, the raw record edits, the PHRED table, the two BAMs of the load
(model.py:214-285) and the CLI options around it."""
import gzip
import os
import struct

import numpy as np
import pytest

from conftest import GOLD, ROOT


def _records(path):
    from telescope_amd import loader
    _, recs, header = loader.read_bam(path, raw=True)
    return [s.raw for s in recs], header


def test_bgzf_bam_round_trip_through_read_bam(tmp_path):
    from telescope_amd import bam_out, loader
    recs, header = _records(os.path.join(GOLD, 'loader_mixed.bam'))
    out = str(tmp_path / 'rt.bam')
    many = recs * 3000                                       # several 64 KiB blocks
    with bam_out.BamWriter(out, header) as w:
        for r in many:
            w.write(r)
    data = open(out, 'rb').read()
    assert data.endswith(bam_out.BGZF_EOF)
    p = 0
    while p < len(data):                                     # every block: a BGZF member of at most 64 KiB
        assert data[p:p + 4] == b'\x1f\x8b\x08\x04' and data[p + 12:p + 14] == b'BC'
        bsize = struct.unpack_from('<H', data, p + 16)[0] + 1
        assert bsize <= 1 << 16
        p += bsize
    assert p == len(data)
    got, h2 = _records(out)
    assert got == many and h2 == header
    refs, segs = loader.read_bam(out)                        # the default path reads it too
    assert refs == ['chrA', 'chrB'] and sum(1 for _ in segs) == len(many)
    assert gzip.decompress(data)[:4] == b'BAM\x01'


def test_set_tag_replaces_and_appends_like_pysam():
    from telescope_amd import bam_out
    recs, _ = _records(os.path.join(GOLD, 'loader_mixed.bam'))
    r = recs[0]
    assert [t for t, *_ in bam_out.iter_tags(r)] == ['NM', 'AS', 'XS', 'ZB']
    r2 = bam_out.set_tag(r, 'ZB', 'L1,L2')                   # a B array replaced by a Z string, at the end
    r2 = bam_out.set_tag(r2, 'NM', 7)
    r2 = bam_out.set_tag(r2, 'XP', 100)
    r2 = bam_out.set_tag(r2, 'XQ', -3)
    r2 = bam_out.set_tag(r2, 'XR', 70000)
    assert bam_out.record_text(r2).split('\t')[3:] == ['AS:i:-5', 'XS:Z:note', 'ZB:Z:L1,L2', 'NM:C:7', 'XP:C:100', 'XQ:c:-3',
                                                       'XR:I:70000']
    assert r2[:bam_out._aux_start(r)] == r[:bam_out._aux_start(r)]           # nothing before the tags is touched
    r3 = bam_out.set_mapq(bam_out.set_flag(r2, 0x100), 42)
    assert bam_out.flag_of(r3) == 0x100 and r3[9] == 42 and r3[10:] == r2[10:14] + r3[14:16] + r2[16:]


def test_phred_table_equals_numpys_expression():
    from telescope_amd import bam_out
    tab = bam_out.phred_table()
    assert 150 <= len(tab) <= 161 and np.all(np.diff(tab) >= 0)
    for p, q in ((0.9, 10), (0.999999, 60), (0, 0), (1, 255), (1.0000000000000002, 255)):
        assert bam_out.phred_lookup([p])[0] == q == bam_out.phred_scalar(p)
    bits = tab.view(np.uint64).astype(np.int64)
    near = np.concatenate([(bits + d) for d in range(-2, 3)])
    near = near[(near >= 0) & (near < int(np.float64(1.0).view(np.uint64)))].astype(np.uint64).view(np.float64)
    rng = np.random.default_rng(8)
    ps = np.concatenate([near, rng.random(1_000_000), 1 - rng.random(1000) * 1e-12])
    want = np.array([bam_out.phred_scalar(p) for p in ps])
    assert np.array_equal(bam_out.phred_lookup(ps, tab), want)


def test_update_pair_restates_update_sam():
    """model.py:495-518 on one pair from a tag word: SEC, PRI assigned, PRI high / low"""
    from telescope_amd import bam_out
    recs, _ = _records(os.path.join(GOLD, 'loader_mixed.bam'))
    pair = recs[6:8]                                          # f04, a proper pair
    sec = bam_out.update_pair(pair, 'SEC', 0)
    assert all(bam_out.flag_of(r) & 0x100 and r[9] == 0 and bam_out.get_tag(r, 'YC') == '248,248,248' for r in sec)
    for z, assigned, yc, sec_flag in ((0.95, 1, '217,95,2', 0), (0.5, 0, '230,171,2', 0x100), (0.125, 0, '209,236,228', 0x100)):
        w = int(bam_out.tag_word(np.array([z]), np.array([assigned]))[0])
        out = bam_out.update_pair([bam_out.set_flag(r, bam_out.flag_of(r) | 0x100) for r in pair], 'PRI', w)
        for r in out:
            assert r[9] == bam_out.phred_scalar(z) and bam_out.get_tag(r, 'XP') == int(round(z * 100))
            assert bam_out.get_tag(r, 'YC') == yc and bam_out.flag_of(r) & 0x100 == sec_flag
            assert [t for t, *_ in bam_out.iter_tags(r)][-2:] == ['XP', 'YC']


def _run_cli(argv):
    from telescope_amd import cli
    return cli.main(argv)


def test_assign_updated_sam_skip_em_writes_other_and_tmp_bams(tmp_path):
    """model.py:214-285: unmapped (SU: alns[0] only) and no-overlap fragments go to -other.bam unchanged, the pairs of every overlapping
    fragment to -tmp_tele.bam with ZF / ZT / ZB (set_tag: the input's B-array ZB is replaced and moves to the end); no updated BAM
    with --skip_em."""
    from telescope_amd import bam_out, loader
    out = str(tmp_path / 'o')
    assert _run_cli(['assign', os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf'), '--updated_sam',
                     '--skip_em', '--outdir', out, '--quiet']) == 0
    assert sorted(os.listdir(out)) == ['telescope-checkpoint.npz', 'telescope-other.bam', 'telescope-tmp_tele.bam']
    inp, header = _records(os.path.join(GOLD, 'loader_mixed.bam'))
    other, h1 = _records(os.path.join(out, 'telescope-other.bam'))
    tmp, h2 = _records(os.path.join(out, 'telescope-tmp_tele.bam'))
    assert h1 == header and h2 == header
    names = lambda rs: [bam_out.qname_of(r) for r in rs]   # noqa: E731
    assert names(other) == ['f03', 'f07', 'f07', 'f10', 'f10', 'f12'] and all(r in inp for r in other)
    assert sorted(set(names(tmp))) == ['f01', 'f02', 'f04', 'f05', 'f06', 'f08', 'f09', 'f11', 'f13', 'f14', 'f15', 'f16', 'f17',
                                       'f18']
    assert len(tmp) + len(other) == len(inp)
    txt = {}
    for r in tmp:
        txt.setdefault(bam_out.qname_of(r), []).append(bam_out.record_text(r).split('\t', 3)[3])
    assert txt['f08'] == ['NM:C:0\tAS:i:-7\tXS:Z:note\tZF:Z:L1\tZT:Z:PRI\tZB:Z:L1', 'NM:C:0\tXS:Z:note\tZB:B:s,1,2']    # unmapped mate: untouched
    assert txt['f11'] == ['NM:C:0\tAS:i:-15\tXS:Z:note\tZF:Z:L1\tZT:Z:SEC\tZB:Z:L1',
                          'NM:C:0\tAS:i:-4\tXS:Z:note\tZF:Z:L1\tZT:Z:PRI\tZB:Z:L1',
                          'NM:C:0\tAS:i:-6\tXS:Z:note\tZF:Z:L2\tZT:Z:PRI\tZB:Z:L1']
    assert all(t.endswith('ZB:Z:L2,L3') for t in txt['f18'])                 # a score tie: both top features
    assert [bam_out.flag_of(r) for r in tmp if bam_out.qname_of(r) == 'f06'] == [99, 147, 323]   # r1, r2, then the lone read


def test_assign_without_updated_sam_writes_no_bam(tmp_path):
    out = str(tmp_path / 'o')
    assert _run_cli(['assign', os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf'), '--skip_em',
                     '--outdir', out, '--quiet']) == 0
    assert os.listdir(out) == ['telescope-checkpoint.npz']


def test_bulk_assign_accepts_tempdir_and_annotation_class():
    from telescope_amd import cli
    a = cli.build_parser().parse_args(['assign', 'x.bam', 'y.gtf', '--tempdir', '/tmp', '--annotation_class', 'htseq',
                                       '--updated_sam'])
    assert a.tempdir == '/tmp' and a.annotation_class == 'htseq' and a.updated_sam
    s = cli.build_parser().parse_args(['sc', 'assign', 'x.bam', 'y.gtf', '--tempdir', '/tmp', '--updated_sam'])
    assert s.tempdir == '/tmp' and s.annotation_class == 'intervaltree' and s.updated_sam


@pytest.mark.parametrize('sc', [False, True])
def test_updated_sam_is_refused_when_row_sharded(tmp_path, monkeypatch, sc):
    monkeypatch.setenv('WORLD_SIZE', '2')
    argv = (['sc'] if sc else []) + ['assign', os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf'),
                                     '--updated_sam', '--outdir', str(tmp_path), '--quiet']
    with pytest.raises(SystemExit) as e:
        _run_cli(argv)
    assert 'WORLD_SIZE' in str(e.value)
    assert os.listdir(str(tmp_path)) == []


def test_ncpu_is_still_refused(tmp_path):
    with pytest.raises(SystemExit):
        _run_cli(['assign', os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf'), '--ncpu', '2',
                  '--outdir', str(tmp_path), '--quiet'])


def test_header_gets_one_pg_line_with_a_unique_id():
    from telescope_amd import bam_out
    t = bam_out.header_with_pg('@HD\tVN:1.6\n', '1.0', 'telescope assign a b')
    assert t == '@HD\tVN:1.6\n@PG\tID:telescope\tPN:telescope\tVN:1.0\tCL:telescope assign a b\n'
    t = bam_out.header_with_pg('@HD\tVN:1.6\n@PG\tID:telescope\tPN:x\n@PG\tID:telescope.1\tPN:x', '1.0', 'c')
    assert t.endswith('@PG\tID:telescope.1\tPN:x\n@PG\tID:telescope.2\tPN:telescope\tVN:1.0\tCL:c\n')
