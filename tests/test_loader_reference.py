"""Host side of the device loader (no GPU): the stage reference is tied to the fixture the reference program produced, the fuzz
generator holds every situation it promises, tsem_bam_scan walks the record chain like the Python reader, the command line takes
`--loader`, and the record code of the kernels — the same functions, compiled as an ordinary host program under the address and
undefined-behaviour sanitizers — reads nothing outside its input, whole, truncated or damaged, and agrees with the Python loader."""
import functools
import os
import random

import numpy as np
import pytest

import _bam_fuzz as fuzz
import _loader_reference as lref
from _loader_reference import FIXTURES, fixture_paths
from conftest import GOLD

FIELDS = ['total_fragments', 'pair_mapped', 'pair_mixed', 'single_mapped', 'unmapped', 'unique', 'ambig', 'overlap_unique', 'overlap_ambig']


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('loader_reference'))


@functools.lru_cache(maxsize=None)
def _case(seed, directory):
    return fuzz.make_case(seed, directory)


@pytest.mark.parametrize('mode', ['None', 'F', 'R', 'FR', 'RF'])
def test_reference_equals_the_reference_programs_fixture(mode):
    ref, _ann = lref.reference(*fixture_paths('loader_mixed'), stranded_mode=mode)
    exp = np.load(os.path.join(GOLD, 'loader_mixed_expected.npz'), allow_pickle=False)
    g = lambda k: exp['%s_%s' % (mode, k)]
    out = ref.result
    raw = out['raw_scores'].tocsr().copy()
    raw.sort_indices()
    assert tuple(raw.shape) == tuple(int(x) for x in g('shape'))
    assert np.array_equal(raw.indptr, g('indptr')) and np.array_equal(raw.indices, g('indices')) and np.array_equal(raw.data, g('data'))
    assert list(out['read_index']) == list(g('rows')) and list(out['feat_index']) == list(g('cols'))
    assert [int(out['run_info'][f]) for f in FIELDS] == g('info').tolist()
    assert list(out['score_range']) == g('score_range').tolist()
    # ... and the stages add up to it: every fragment with a feature has its maps, in the order of the rows
    rows = [ref.segments[b['first']].qname for b in ref.bundles if b['cls'] >= 3]
    assert list(dict.fromkeys(rows)) == [r for r in out['read_index']]
    assert sum(b['code'] in (0, 2) for b in ref.bundles) == out['run_info']['unmapped']


def test_fuzz_cases_hold_every_situation(workdir):
    for seed in range(20):
        c = _case(seed, workdir)
        missing = [s for s in fuzz.SITUATIONS if c.situations[s] < 1]
        assert not missing, 'seed %d lacks %s' % (seed, missing)
        assert 200 <= c.n_records <= 2000
    again = os.path.join(workdir, 'again')
    os.makedirs(again, exist_ok=True)
    a, b = _case(3, workdir), fuzz.make_case(3, again)
    assert open(a.bam, 'rb').read() == open(b.bam, 'rb').read()                  # seeded: the same bytes again


def _scan_inputs(workdir):
    for name in FIXTURES:
        yield fixture_paths(name)[0]
    for seed in range(4):
        yield _case(seed, workdir).bam


def test_bam_scan_gives_the_python_offsets_whole_and_cut(workdir):
    from telescope_amd import _lib
    rng = random.Random(5)
    for bam in _scan_inputs(workdir):
        _refs, data, off = lref.inflated_records(bam)
        got, used = _lib.bam_scan(data)
        assert np.array_equal(got, off) and used == len(data), bam
        got, used = _lib.bam_scan(data, cap=3)                                   # a full offsets array ends the walk as well
        assert np.array_equal(got, off[:4]) and used == off[3]
        for _ in range(25):                                                      # a cut anywhere: the partial record stays behind
            cut = rng.randrange(len(data))
            got, used = _lib.bam_scan(data[:cut])
            k = int(np.searchsorted(off, cut, side='right')) - 1
            assert used == off[k] and np.array_equal(got, off[:k + 1]), (bam, cut)
        for i in (1, len(off) // 2):                                             # ... also 1, 2, 3 bytes into a size field and right behind it
            for d in (0, 1, 3, 4):
                got, used = _lib.bam_scan(data[:int(off[i]) + d])
                assert used == off[i] and len(got) == i + 1
    got, used = _lib.bam_scan(b'')
    assert got.tolist() == [0] and used == 0


def test_bam_scan_refuses_a_block_size_below_32(workdir):
    from telescope_amd import _lib
    _refs, data, off = lref.inflated_records(fixture_paths('loader_mixed')[0])
    o = int(off[5])
    bad = data[:o] + (31).to_bytes(4, 'little') + data[o + 4:]
    with pytest.raises(_lib.EngineError) as e:
        _lib.bam_scan(bad)
    assert e.value.code == _lib.ERR_ARG and 'block_size 31' in str(e.value) and 'record 5' in str(e.value)
    with pytest.raises(_lib.EngineError):
        _lib.bam_scan(data[:o] + (-7 & 0xffffffff).to_bytes(4, 'little') + data[o + 4:])


def test_cli_takes_the_loader_option_and_refuses_updated_sam(tmp_path, capsys):
    from telescope_amd import cli
    ap = cli.build_parser()
    for argv in (['assign', 'a.bam', 'a.gtf'], ['sc', 'assign', 'a.bam', 'a.gtf']):
        assert ap.parse_args(argv).loader == 'python'
        assert ap.parse_args(argv + ['--loader', 'device']).loader == 'device'
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ['--loader', 'pysam'])
        with pytest.raises(SystemExit) as e:                                     # before anything is read: the files do not exist
            cli.main(argv[:-2] + [str(tmp_path / 'none.bam'), str(tmp_path / 'none.gtf'), '--loader', 'device', '--updated_sam',
                                  '--outdir', str(tmp_path / 'o')])
        assert '--loader device with --updated_sam is not supported' in str(e.value)
        assert not os.path.exists(str(tmp_path / 'o'))
    capsys.readouterr()


def test_loader_keyword_is_checked():
    from telescope_amd import loader
    ann = loader.Annotation(fixture_paths('loader_mixed')[1], 'locus', 'None')
    with pytest.raises(ValueError):
        loader.load_alignment(fixture_paths('loader_mixed')[0], ann, loader='pysam')
    with pytest.raises(ValueError):
        loader.load_alignment(fixture_paths('loader_mixed')[0], ann, loader='device', updated_sam=('a', 'b'))


# ------------------------------------------------------------------------------------ the stand-alone sanitizer program
@pytest.fixture(scope='module')
def host_program(workdir):
    return lref.build_host_program(workdir)


def _decoded_lines(lines):
    return [[int(x) for x in l.split()[2:]] for l in lines if l.startswith('R ')]


def _check_decode(lines, bam, btag, utag, data, off):
    """the program's per-record lines against read_bam"""
    from telescope_amd import loader
    _refs, records = loader.read_bam(bam, btag, umi_tag=utag)
    rows = _decoded_lines(lines)
    n = 0
    for i, (s, r) in enumerate(zip(records, rows)):
        ref_id, pos, nref, npos, atlen, flag, l_rn, n_cig, _l_seq, AS, bits, bco, bcl, uo, ul, status = r
        assert status == 0
        assert (ref_id, pos, nref, npos, atlen, flag, l_rn, n_cig) == (s.ref_id, s.pos, s.nref, s.npos, abs(s.tlen), s.flag, len(s.qname) + 1,
                                                                      len(s.cigar)), i
        assert (AS if bits & 1 else None) == s.AS, i
        o = int(off[i])
        assert (None if bco < 0 else data[o + bco:o + bco + bcl].decode()) == s.bc and (None if uo < 0 else data[o + uo:o + uo + ul].decode()) == s.umi
        n += 1
    assert n == len(rows) == len(off) - 1


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_host_program_decodes_the_fixtures_like_read_bam(name, host_program, workdir):
    bam, _gtf = fixture_paths(name)
    btag, utag = FIXTURES[name]
    _refs, data, off = lref.inflated_records(bam)
    path = os.path.join(workdir, name + '.records')
    with open(path, 'wb') as fh:
        fh.write(data)
    lines, _m, _s = lref.host_run(host_program, path, btag, utag)
    assert lines[0] == 'scan %d %d' % (len(off) - 1, len(data)) and lines[-1] == 'status 0'
    _check_decode(lines, bam, btag, utag, data, off)


@pytest.mark.parametrize('name,mode', [('loader_mixed', 'None'), ('loader_mixed', 'FR'), ('loader_mixed', 'R'), ('sc_umi', 'None'),
                                       ('updated_mixed', 'None'), ('fuzz0', 'None'), ('fuzz1', 'F'), ('fuzz2', 'RF')])
def test_host_program_stages_equal_the_reference(name, mode, host_program, workdir):
    """all four stages on the host (the kernels' own functions in loops): per-stage equality with the Python loader"""
    if name.startswith('fuzz'):
        c = _case(int(name[4:]), workdir)
        bam, gtf, btag, utag, cap, n_host = c.bam, c.gtf, 'CB', 'UB', fuzz.RECORD_CAP, c.expected_fallbacks
    else:
        (bam, gtf), (btag, utag), cap, n_host = fixture_paths(name), FIXTURES[name], 4096, 0
    ref, ann = lref.reference(bam, gtf, mode, btag, utag)
    rec, annot, out = (os.path.join(workdir, '%s_%s.%s' % (name, mode, x)) for x in ('records', 'annot', 'out'))
    with open(rec, 'wb') as fh:
        fh.write(ref.inflated)
    lref.write_annotation(ann, ref.refs, annot)
    lines, mat, st = lref.host_run(host_program, rec, btag, utag, annot, ann.run_stranded, mode[0] == 'F', mode[-1] == 'F', 0.2, cap, out)
    assert st == (0, -1) and lines[-1] == 'status 0'
    over_cap = [b['first'] for b in ref.bundles if b['n'] > cap]
    hosted = np.flatnonzero(mat[28] == 5).tolist()
    assert len(hosted) == n_host and set(over_cap) <= set(hosted)
    lref.compare_stages(ref, ann, mat, host_expected=hosted)


def test_host_program_survives_truncated_and_damaged_records(host_program, workdir):
    """truncated and bit-flipped copies: the run must end clean under the sanitizers, whatever it reports"""
    rng = random.Random(11)
    inputs = [fixture_paths('loader_mixed'), fixture_paths('sc_umi'), (_case(0, workdir).bam, _case(0, workdir).gtf)]
    for k, (bam, gtf) in enumerate(inputs):
        from telescope_amd import loader
        ann = loader.Annotation(gtf, 'locus', 'FR')
        refs, data, off = lref.inflated_records(bam)
        annot = os.path.join(workdir, 'damaged_%d.annot' % k)
        lref.write_annotation(ann, refs, annot)
        copies = [data[:rng.randrange(len(data))] for _ in range(6)]
        for _ in range(30):
            b = bytearray(data)
            for _ in range(rng.choice([1, 1, 2, 8])):
                i = rng.randrange(len(b))
                b[i] ^= 1 << rng.randrange(8)
            copies.append(bytes(b))
        for i in (3, len(off) // 2):                                              # aimed damage: the counts and lengths of one record
            o = int(off[i])
            for field, width in ((12, 1), (16, 2), (20, 4)):                      # l_read_name, n_cigar, l_seq
                b = bytearray(data)
                b[o + field:o + field + width] = b'\xff' * width if width < 4 else (0x7fffffff).to_bytes(4, 'little')
                copies.append(bytes(b))
        for j, c in enumerate(copies):
            path = os.path.join(workdir, 'damaged_%d_%d.records' % (k, j))
            with open(path, 'wb') as fh:
                fh.write(c)
            lines, _mat, _st = lref.host_run(host_program, path, 'CB', 'UB', annot, 1, 0, 1, 0.2, 16, path + '.out')
            assert lines and (lines[0].startswith('scan ') or lines[0].startswith('scan error: tsem_bam_scan: record '))
            os.remove(path)
