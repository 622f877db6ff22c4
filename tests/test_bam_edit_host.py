"""The record rewriting of `--updated_sam --rewrite device` without a GPU: the edit body of telescope_amd/csrc/tsem_bam_edit.h in a
stand-alone program under the address and undefined-behaviour sanitizers (tests/c_host/bam_edit_check.cc: every record in a heap block
of exactly its size, every output in one of exactly the sized length) against bam_out.set_tag / set_flag / set_mapq / update_pair, byte
for byte; the CLI's refusals and defaults; BamWriter's framed-stream write."""
import filecmp
import os
import random
import struct

import pytest

import _bam_edit_reference as ed
from _bam_edit_reference import KEEP, PRI, SEC
from _bgzf_reference import FIXTURE_BAMS, GOLD
from telescope_amd import bam_out, cli, loader

WORDS = [ed.word(KEEP), ed.word(SEC), ed.word(SEC, 77, 50, True, True),
         ed.word(PRI, 0, 0), ed.word(PRI, 255, 100, True, True), ed.word(PRI, 0, 100, False, True), ed.word(PRI, 255, 0, True, False),
         ed.word(PRI, 13, 19, False, False), ed.word(PRI, 160, 99, True, False)]
# locus names of 1 and of 60 characters, a no_feature_key that is not the default (the last name)
LOAD_NAMES = ['L', 'M' * 60, 'HERV_3p12', 'x', '__none_of_them']
# (feat, pri, mfeat, mas): ZB with three mappings tied at the top score and one below; one mapping; the no_feature_key as ZF and in ZB
LOADS = [(1, True, [0, 1, 2, -1], [50, 50, 50, 49]), (0, False, [0], [7]), (-1, True, [2, -1, 3, 1], [-3, -3, -4, -3]),
         (3, False, [3, -1], [0, 0])]


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    return ed.build_host_program(str(tmp_path_factory.mktemp('bam_edit')))


def _load_expected(rec, feat, pri, mfeat, mas):
    return ed.loaded(rec, LOAD_NAMES[feat], pri, ed.zb_of(LOAD_NAMES, mfeat, mas))


def test_edit_built_cases_update_stage(exe, tmp_path):
    """no aux at all; the only aux field is one to strip; ZF ZT ZB XP YC first, middle, last, twice, as Z A C i f B; XP 0 and 100, MAPQ 0
    and 255; a SEC pair's XP stays where it is"""
    recs = [(label, ed.record('q%d' % k, flag, aux)) for k, (label, aux) in enumerate(ed.built_aux()) for flag in (0x53, 0x100 | 0x10)]
    cases, want, labels = [], [], []
    for label, rec in recs:
        for w in WORDS:
            cases.append(ed.case_update(rec, w)); want.append(ed.updated(rec, w)); labels.append((label, hex(w)))
    got = ed.host_run(exe, cases, str(tmp_path))
    for g, w, l in zip(got, want, labels):
        assert g == w, (l, g if isinstance(g, int) else bam_out.record_text(g), bam_out.record_text(w))
    # the SEC pair's XP: still in front of the fields behind it
    rec = ed.record('s', 0, ed.aux_as('XP', 'C') + ed.OTHERS[0] + ed.aux_as('YC', 'Z') + ed.OTHERS[1])
    (g,) = ed.host_run(exe, [ed.case_update(rec, ed.word(SEC))], str(tmp_path), 'sec')
    assert [t[0] for t in bam_out.iter_tags(g)] == ['XP', 'AS', 'NM', 'YC'] and bam_out.get_tag(g, 'XP') == 7
    assert bam_out.flag_of(g) == 0x100 and g[9] == 0 and bam_out.get_tag(g, 'YC') == bam_out.YC_SEC


def test_edit_built_cases_load_stage(exe, tmp_path):
    """the same aux lists through ZF / ZT / ZB: names of 1 and 60 characters, a non-default no_feature_key, three mappings tied at the top"""
    cases, want, labels = [], [], []
    for k, (label, aux) in enumerate(ed.built_aux()):
        rec = ed.record('frag%d' % k, 0x63, aux)
        for load in LOADS:
            cases.append(ed.case_load(rec, LOAD_NAMES, *load)); want.append(_load_expected(rec, *load)); labels.append((label, load))
    got = ed.host_run(exe, cases, str(tmp_path))
    for g, w, l in zip(got, want, labels):
        assert g == w, (l, g if isinstance(g, int) else bam_out.record_text(g), bam_out.record_text(w))
    assert bam_out.get_tag(want[0], 'ZB') == 'L,' + 'M' * 60 + ',HERV_3p12' and bam_out.get_tag(want[2], 'ZF') == '__none_of_them'


def test_edit_body_flag_masks_mapq_and_any_append(exe, tmp_path):
    rng = random.Random(5)
    cases, want = [], []
    for k, (label, aux) in enumerate(ed.built_aux()):
        rec = ed.record('e%d' % k, rng.randrange(1 << 16), aux, mapq=rng.randrange(256))
        f_and, f_or, mapq = rng.randrange(1 << 16), rng.randrange(1 << 16), rng.choice([-1, 0, 255, rng.randrange(256)])
        strip = rng.sample(ed.NAMES + ('AS', 'XB'), rng.randrange(0, 5))
        new = [(n, rng.choice(['v', 3, -3, 70000, 1.5, ''])) for n in strip[:rng.randrange(0, len(strip) + 1)]]
        w = bam_out.set_flag(rec, (bam_out.flag_of(rec) & f_and) | f_or)
        w = bam_out.set_mapq(w, mapq) if mapq >= 0 else w
        for n in strip:
            w = bam_out.set_tag(w, n, 0)
        a = w[:len(w) - 4 * len(strip)]                         # (every set_tag appended XXC\0: cut them off again)
        app = b''.join(bam_out.encode_tag(n, v) for n, v in new)
        cases.append(ed.case_edit(rec, f_and, f_or, mapq, strip, app)); want.append(a + app)
    assert ed.host_run(exe, cases, str(tmp_path)) == want


def test_edit_every_fixture_record(exe, tmp_path):
    """every record of the fixture BAMs through the update stage (the words in rotation) and through the load stage"""
    for name in FIXTURE_BAMS:
        _, recs, _ = loader.read_bam(os.path.join(GOLD, name), raw=True)
        cases, want = [], []
        for k, s in enumerate(recs):
            w, load = WORDS[k % len(WORDS)], LOADS[k % len(LOADS)]
            cases += [ed.case_update(s.raw, w), ed.case_load(s.raw, LOAD_NAMES, *load)]
            want += [ed.updated(s.raw, w), _load_expected(s.raw, *load)]
        assert cases
        got = ed.host_run(exe, cases, str(tmp_path), name)
        bad = [k for k, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (name, bad[:5])


def test_edit_a_record_cut_anywhere_is_refused_not_read_past(exe, tmp_path):
    """a record truncated at every length (its block_size rewritten to match, so the walk itself must find the end): a status code or
    a valid rewrite, never a read behind the block"""
    rec = ed.record('cut', 0, ed.aux_as('ZF', 'Z') + ed.OTHERS[3] + ed.aux_as('YC', 'B') + ed.OTHERS[2], cigar=((5, 0), (3, 1)))
    cases = []
    for n in range(32, len(rec)):
        for w in (ed.word(SEC), ed.word(PRI, 1, 2)):
            cases.append(ed.case_update(rec[:n], w))
    # a block_size that disagrees with the record's length, an unknown aux type, a negative B count
    wrong = struct.pack('<iq', 1, len(rec) + 4) + struct.pack('<i', len(rec) + 1) + rec + struct.pack('<I', ed.word(SEC))
    got = ed.host_run(exe, cases + [wrong, ed.case_update(ed.record('t', 0, b'XX?\x00'), ed.word(SEC)),
                                    ed.case_update(ed.record('b', 0, b'XBBc' + struct.pack('<i', -1)), ed.word(SEC))], str(tmp_path))
    assert got[-3:] == [-1, -9, -8]
    assert any(isinstance(g, int) for g in got[:-3]) and all(isinstance(g, bytes) or -9 <= g <= -1 for g in got)
    for c, g in zip(cases, got):
        if isinstance(g, bytes):                                 # cut on a field boundary: a valid record, rewritten as bam_out does
            n = struct.unpack_from('<q', c, 4)[0] - 4
            assert g == ed.updated(rec[:n], struct.unpack_from('<I', c, len(c) - 4)[0])


# ------------------------------------------------------------------------------------------- the whole load stage on the host
def _host_load_equals_python(exe, d, bam, gtf, mode, cap, no_feature_key='__no_feature'):
    ann = loader.Annotation(gtf, 'locus', mode)
    want = (os.path.join(d, 'py-other.bam'), os.path.join(d, 'py-tmp.bam'))
    loader.load_alignment(bam, ann, no_feature_key, stranded_mode=mode, updated_sam=want)
    other, tmp, hosted = ed.host_load(exe, bam, ann, mode, no_feature_key, cap, d)
    assert other == ed.record_stream(want[0]) and tmp == ed.record_stream(want[1])
    return hosted


@pytest.mark.parametrize('name,mode', [('loader_mixed', 'None'), ('loader_mixed', 'RF'), ('loader_mixed', 'F'), ('sc_mixed', 'None'),
                                       ('updated_mixed', 'None'), ('updated_mixed', 'FR')])
def test_load_stage_on_the_host_writes_the_python_loaders_streams(exe, tmp_path, name, mode):
    """plan, size, scan and write in plain loops under the sanitizers, the outputs in blocks of exactly the scans' totals"""
    import _loader_reference as lr
    bam, gtf = lr.fixture_paths(name)
    assert _host_load_equals_python(exe, str(tmp_path), bam, gtf, mode, 4096, '__no_feature' if mode == 'None' else 'nothing here') == 0


@pytest.mark.parametrize('seed', range(6))
def test_load_stage_on_the_host_fuzz(exe, tmp_path, seed):
    import _bam_fuzz as fuzz
    case = fuzz.make_case(seed, str(tmp_path))
    mode = ['None', 'RF', 'R', 'FR', 'F'][seed % 5]
    assert _host_load_equals_python(exe, str(tmp_path), case.bam, case.gtf, mode, fuzz.RECORD_CAP) == fuzz.EXPECTED_FALLBACKS


# ------------------------------------------------------------------------------------------------------------------ the CLI
def _assign(*more):
    return ['assign', os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf')] + list(more)


def test_cli_rewrite_defaults_to_host():
    for argv in (_assign(), ['sc'] + _assign()):
        assert cli.build_parser().parse_args(argv).rewrite == 'host'
    assert cli.build_parser().parse_args(_assign('--rewrite', 'device')).rewrite == 'device'
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(_assign('--rewrite', 'gpu'))


@pytest.mark.parametrize('sc', [False, True])
def test_cli_rewrite_device_refusals_come_before_anything_is_read(tmp_path, sc):
    out = str(tmp_path / 'never')
    head = ['sc'] if sc else []
    with pytest.raises(SystemExit) as e:
        cli.main(head + _assign('--rewrite', 'device', '--loader', 'device', '--outdir', out))
    assert '--rewrite device' in str(e.value) and '--updated_sam' in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(head + _assign('--rewrite', 'device', '--updated_sam', '--outdir', out))
    assert '--rewrite device' in str(e.value) and '--loader device' in str(e.value)
    with pytest.raises(SystemExit) as e:                         # the old refusal, its message unchanged at the front
        cli.main(head + _assign('--loader', 'device', '--updated_sam', '--outdir', out))
    assert str(e.value).startswith('telescope assign: --loader device with --updated_sam is not supported')
    assert not os.path.exists(out)


def test_loader_keeps_its_refusal_without_rewrite_device(tmp_path):
    ann = loader.Annotation(os.path.join(GOLD, 'loader_mixed.gtf'), 'locus', 'None')
    with pytest.raises(ValueError, match='the device loader does not write the BAMs of --updated_sam'):
        loader.load_alignment(os.path.join(GOLD, 'loader_mixed.bam'), ann, loader='device', updated_sam=(str(tmp_path / 'o'), str(tmp_path / 't')))
    with pytest.raises(ValueError, match="rewrite"):
        loader.load_alignment(os.path.join(GOLD, 'loader_mixed.bam'), ann, rewrite='device')
    assert not os.listdir(str(tmp_path))


# ----------------------------------------------------------------------------------------------------------- BamWriter
@pytest.mark.parametrize('seed', range(4))
def test_bamwriter_framed_stream_in_arbitrary_pieces(tmp_path, seed):
    """a framed stream written in arbitrary pieces (empty ones, pieces that end inside a block_size, one larger than three BGZF
    blocks) gives the same file as the same records written one by one"""
    rng = random.Random(seed)
    header = dict(text='@HD\tVN:1.6\n', refs_block=struct.pack('<i', 0))
    recs = [ed.record('n%d' % k, k & 0xffff, b'XYZ' + bytes(rng.randrange(1, 256) for _ in range(rng.randrange(0, 900))) + b'\x00')
            for k in range(700)]
    one, two = str(tmp_path / 'one.bam'), str(tmp_path / 'two.bam')
    with bam_out.BamWriter(one, header) as w:
        for r in recs:
            w.write(r)
    stream = b''.join(ed.frame(r) for r in recs)
    assert len(stream) > 4 * 0xff00
    cuts = sorted(rng.randrange(len(stream) + 1) for _ in range(40)) + [len(stream)]
    cuts = [0, 0, 1, 3] + [c for c in cuts if c > 3 and not 1000 < c < 1000 + 3 * 0xff00 + 17] + [len(stream)]
    with bam_out.BamWriter(two, header) as w:
        for a, b in zip(cuts[:-1], cuts[1:]):
            w.write_framed(memoryview(stream)[a:b] if (a + b) % 2 else stream[a:b])
    assert filecmp.cmp(one, two, shallow=False)
    got = [s.raw for s in loader.read_bam(two, raw=True)[1]]
    assert got == recs
