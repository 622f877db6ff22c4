"""`--updated_sam --loader device --rewrite device`, `-m gpu`: the three BAMs with their records rewritten on the GPU are the Python
path's FILES (filecmp: both routes write through bam_out.BgzfWriter, so equal record streams give equal files) — the load stage
(other, tmp), its chunking, BAMs built for the places where the rewrite can go wrong, the update stage end to end through the CLI,
and the error path of a damaged tmp BAM.  No tolerance anywhere."""
import filecmp
import os
import re
import shutil
import struct

import numpy as np
import pytest

import _bam_edit_reference as ed
import _bam_fuzz as fuzz
import _loader_reference as lr
from telescope_amd import bam_out, cli, loader
from telescope_amd import loader_device as ld

pytestmark = pytest.mark.gpu
_PY = {}


@pytest.fixture(autouse=True)
def _no_torch_stays_in_this_test(monkeypatch):
    """a single-process command-line run sets TSEM_NO_TORCH for itself (cli.warm_device, cli.build_model): in-process here, so it must
    not stay behind for the rank processes that later tests start (they load torch's HIP runtime first)"""
    monkeypatch.setenv('TSEM_NO_TORCH', '1')


def _paths(d, tag):
    return os.path.join(str(d), tag + '-other.bam'), os.path.join(str(d), tag + '-tmp.bam')


def _python_load(key, d, bam, ann, **kw):
    """the Python loader's dict and two BAMs, once per module and key"""
    if key not in _PY:
        out = _paths(d, 'py')
        _PY[key] = (loader.load_alignment(bam, ann, updated_sam=out, **kw), out)
    return _PY[key]


def _same_files(got, want):
    for g, w in zip(got, want):
        assert filecmp.cmp(g, w, shallow=False), (g, [bam_out.record_text(s.raw) for s in loader.read_bam(g, raw=True)[1]][:3],
                                                  [bam_out.record_text(s.raw) for s in loader.read_bam(w, raw=True)[1]][:3])


def _n_records(path):
    return sum(1 for _ in loader.read_bam(path)[1])


def _check_load(gpu_device, d, key, bam, ann, fallbacks, **kw):
    want, wfiles = _python_load(key, d, bam, ann, **{k: v for k, v in kw.items() if k != 'record_cap'})
    out = _paths(d, 'dev')
    got = loader.load_alignment(bam, ann, updated_sam=out, loader='device', rewrite='device', device=gpu_device, **kw)
    lr.assert_same_load(got, want)
    _same_files(out, wfiles)
    st = ld.LAST_STATS
    assert st['fallbacks'] == fallbacks
    assert (st['records_other'], st['records_tmp']) == (_n_records(out[0]), _n_records(out[1]))
    tab = ld.LAST_TMP_TABLE
    assert len(tab['row']) == len(tab['col']) == len(tab['kind']) == st['records_tmp'] and tab['kind'].dtype == np.uint8
    return got


# ------------------------------------------------------------------------------------------------------------ load stage
@pytest.mark.parametrize('mode', ['None', 'RF', 'R', 'FR', 'F'])
def test_rewrite_load_loader_mixed(gpu_device, tmp_path_factory, mode):
    bam, gtf = lr.fixture_paths('loader_mixed')
    ann = loader.Annotation(gtf, 'locus', mode)
    _check_load(gpu_device, tmp_path_factory.mktemp('lm'), ('loader_mixed', mode), bam, ann, 0, stranded_mode=mode)


@pytest.mark.parametrize('name', ['sc_mixed', 'updated_mixed', 'bundled'])
def test_rewrite_load_fixtures(gpu_device, tmp_path_factory, name):
    bam, gtf = lr.fixture_paths(name)
    ann = loader.Annotation(gtf, 'locus', 'None')
    _check_load(gpu_device, tmp_path_factory.mktemp(name), (name, 'None'), bam, ann, 0, barcode_tag=lr.FIXTURES[name][0])


@pytest.fixture(scope='module')
def fuzz_dir(tmp_path_factory):
    return tmp_path_factory.mktemp('fuzz')


@pytest.mark.parametrize('seed', range(20))
def test_rewrite_load_fuzz(gpu_device, fuzz_dir, tmp_path, seed):
    case = fuzz.make_case(seed, str(fuzz_dir))
    mode = ['None', 'RF', 'R', 'FR', 'F'][seed % 5]
    ann = loader.Annotation(case.gtf, 'locus', mode)
    _check_load(gpu_device, tmp_path, ('fuzz', seed), case.bam, ann, fuzz.EXPECTED_FALLBACKS, stranded_mode=mode, record_cap=fuzz.RECORD_CAP)


@pytest.mark.parametrize('chunk', [dict(chunk_bytes=4096), dict(chunk_bytes=64), dict(max_bundles=1)], ids=['4096', '64', 'one-bundle'])
@pytest.mark.parametrize('which', ['loader_mixed', 0, 1, 7])
def test_rewrite_load_chunking_does_not_change_the_files(gpu_device, fuzz_dir, tmp_path, which, chunk):
    if which == 'loader_mixed':
        (bam, gtf), cap, mode = lr.fixture_paths(which), 4096, 'None'
    else:
        case = fuzz.make_case(which, str(fuzz_dir))
        bam, gtf, cap, mode = case.bam, case.gtf, fuzz.RECORD_CAP, ['None', 'RF', 'R', 'FR', 'F'][which % 5]
    ann = loader.Annotation(gtf, 'locus', mode)
    want, wfiles = _python_load(('fuzz', which) if which != 'loader_mixed' else (which, mode), tmp_path, bam, ann, stranded_mode=mode)
    out = _paths(tmp_path, 'dev')
    got = ld.load_alignment_device(bam, ann, stranded_mode=mode, device=gpu_device, record_cap=cap, updated_sam=out, **chunk)
    lr.assert_same_load(got, want)
    _same_files(out, wfiles)
    assert ld.LAST_STATS['chunks'] > 1


# ------------------------------------------------------------------------------------------------------- built BAMs, end to end
M = lambda n: [(n, 'M')]


def _built_cases():
    e = fuzz.encode
    feat = lambda name, pos=1100, AS=-3, flag=0, aux=b'': e(name, flag, 0, pos, M(50), AS=AS) + aux      # c1:1000-1999 is L_a
    nofeat = lambda name, flag=0: e(name, flag, 0, 60000, M(50), AS=-1)
    su = lambda name: e(name, 4, -1, -1, [])
    cases = {}
    cases['no_feature_anywhere'] = [nofeat('a'), su('b'), nofeat('c'), nofeat('c', 0x100)]
    cases['every_fragment_has_a_feature'] = [feat('a'), feat('b', 3100), feat('c'), feat('c', 3100, flag=0x100)]
    cases['su_bundle_of_several_records'] = [feat('a'), su('u'), su('u'), su('u'), feat('z', 3100)]
    cases['px_unmapped_read_inside_a_feat_bundle'] = [
        feat('a'), e('p', 0x1 | 0x40, 0, 1100, M(50), nref=0, npos=1100, AS=-2), e('p', 0x1 | 0x80 | 0x4, 0, 1100, [], nref=0, npos=1100),
        e('p', 0x1 | 0x40 | 0x100, 0, 3100, M(50), AS=-9)]
    cases['query_name_returns_later'] = [feat('r'), feat('r', 3100, flag=0x100), nofeat('x'), feat('y', 3100), feat('r', 3100, AS=-1),
                                         feat('r', 1200, AS=-1, flag=0x100), feat('r', 1300, AS=-7, flag=0x100)]
    tagged = []
    for k, (_label, aux) in enumerate(ed.built_aux()):                  # ZF ZT ZB XP YC already there: first, middle, last, twice, every type
        n = 't%d' % k
        tagged += [feat(n, 1100, -1, 0, aux), feat(n, 1150, -1, 0x100, aux), feat(n, 1200, -4, 0x100, aux), feat(n, 3100, -1, 0x100, aux),
                   nofeat(n, 0x100) + aux]
    cases['records_that_carry_the_tags_already'] = tagged
    return cases


BUILT = _built_cases()


def _write_built(d, records):
    bam, gtf = os.path.join(str(d), 'built.bam'), os.path.join(str(d), 'built.gtf')
    refs_block = struct.pack('<i', len(fuzz.REFS)) + b''.join(
        struct.pack('<i', len(n) + 1) + n.encode() + b'\x00' + struct.pack('<i', l) for n, l in fuzz.REFS)
    text = '@HD\tVN:1.6\tSO:unsorted\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % x for x in fuzz.REFS)
    with bam_out.BamWriter(bam, dict(text=text, refs_block=refs_block)) as w:
        for r in records:
            w.write(r)
    with open(gtf, 'w') as fh:
        for chrom, s, e, strand, loc in fuzz.GTF_ROWS:
            fh.write('%s\tfuzz\texon\t%d\t%d\t.\t%s\t.\tgene_id "%s"; locus "%s";\n' % (chrom, s, e, strand, loc, loc))
    return bam, gtf


def _same_npz(a, b):
    x, y = np.load(a, allow_pickle=True), np.load(b, allow_pickle=True)
    assert sorted(x.files) == sorted(y.files)
    for k in x.files:
        assert x[k].dtype == y[k].dtype and np.array_equal(x[k], y[k]), k


def _run_both(tmp_path, head, args, more_device=()):
    """the same command with the Python loader and with --loader device --rewrite device: every output file must be identical"""
    dirs = {}
    for route, more in (('python', []), ('device', ['--loader', 'device', '--rewrite', 'device'] + list(more_device))):
        dirs[route] = str(tmp_path / route)
        assert cli.main(head + ['assign'] + args + ['--updated_sam', '--quiet', '--outdir', dirs[route]] + more) == 0
    names = sorted(os.listdir(dirs['python']))
    assert names == sorted(os.listdir(dirs['device'])) and 'telescope-other.bam' in names and 'telescope-tmp_tele.bam' in names
    for f in names:
        a, b = os.path.join(dirs['python'], f), os.path.join(dirs['device'], f)
        if f.endswith('.npz'):
            _same_npz(a, b)
        else:
            assert filecmp.cmp(a, b, shallow=False), f
    return dirs['device'], names


@pytest.mark.parametrize('name', sorted(BUILT))
def test_rewrite_built_bams_end_to_end(gpu_device, tmp_path, name):
    bam, gtf = _write_built(tmp_path, BUILT[name])
    out, names = _run_both(tmp_path, [], [bam, gtf, '--reassign_mode', 'conf'])
    n = {f: _n_records(os.path.join(out, f)) for f in names if f.endswith('.bam')}
    assert ld.LAST_STATS['fallbacks'] == 0
    if name == 'no_feature_anywhere':
        assert n == {'telescope-other.bam': 4, 'telescope-tmp_tele.bam': 0}                 # (nothing overlaps: the run ends before update_sam)
    else:
        assert n['telescope-updated.bam'] == n['telescope-tmp_tele.bam'] > 0
    if name == 'every_fragment_has_a_feature':
        assert n['telescope-other.bam'] == 0
    if name == 'su_bundle_of_several_records':
        assert n['telescope-other.bam'] == 1
    if name == 'px_unmapped_read_inside_a_feat_bundle':
        recs = [s.raw for s in loader.read_bam(os.path.join(out, 'telescope-tmp_tele.bam'), raw=True)[1]]
        assert [bam_out.get_tag(r, 'ZT') for r in recs] == ['PRI', 'PRI', None, 'PRI']
    if name == 'query_name_returns_later':
        tab = ld.LAST_TMP_TABLE
        assert tab['row'].tolist() == [0, 0, 1, 0, 0, 0] and tab['kind'].tolist() == [2, 2, 2, 2, 2, 1]


# ------------------------------------------------------------------------------------------------- update stage, end to end
@pytest.mark.parametrize('mode', ['exclude', 'choose', 'conf'])
@pytest.mark.parametrize('name', ['loader_mixed', 'updated_mixed'])
def test_rewrite_cli_end_to_end(gpu_device, tmp_path, name, mode):
    bam, gtf = lr.fixture_paths(name)
    _, names = _run_both(tmp_path, [], [bam, gtf, '--reassign_mode', mode])
    assert 'telescope-updated.bam' in names and 'telescope-TE_counts.tsv' in names


def test_rewrite_cli_end_to_end_bundled(gpu_device, tmp_path):
    bam, gtf = lr.fixture_paths('bundled')
    _, names = _run_both(tmp_path, [], [bam, gtf, '--reassign_mode', 'exclude'])
    assert 'telescope-updated.bam' in names


def test_rewrite_cli_end_to_end_sc(gpu_device, tmp_path):
    bam, gtf = lr.fixture_paths('sc_mixed')
    _, names = _run_both(tmp_path, ['sc'], [bam, gtf, '--barcode_tag', 'CB'])
    assert 'telescope-updated.bam' in names


def test_rewrite_cli_end_to_end_with_device_inflate(gpu_device, tmp_path):
    bam, gtf = lr.fixture_paths('loader_mixed')
    _, names = _run_both(tmp_path, [], [bam, gtf], more_device=['--inflate', 'device'])
    assert 'telescope-updated.bam' in names


# --------------------------------------------------------------------------------------------------------------- error path
def test_rewrite_update_names_a_truncated_record(gpu_device, tmp_path):
    """a tmp BAM with one record cut short mid-file (its block_size says what is left, so the record chain holds and the walk inside
    the record must find it): ValueError with the record's index and name; one record fewer: an error as well"""
    from test_gpu_updated_sam import _O
    from telescope_amd.run_container import Telescope
    bam, gtf = lr.fixture_paths('loader_mixed')
    o = _O(bam, gtf, str(tmp_path), 'exclude', loader='device', rewrite='device', device=gpu_device)
    ts = Telescope(o)
    ts.load_alignment(loader.Annotation(gtf, 'locus', 'None'))
    np.random.seed(ts.get_random_seed())
    tl, _ = cli.build_model(ts.raw_scores, o)
    tl.em()
    _, segs, header = loader.read_bam(ts.tmp_bam, raw=True)
    recs = [s.raw for s in segs]
    k = next(i for i in range(len(recs) // 2, len(recs)) if bam_out.get_tag(recs[i], 'ZT') in ('PRI', 'SEC'))   # (it ends ... ZB:Z:names NUL)
    assert 0 < k < len(recs) - 1 and list(bam_out.iter_tags(recs[k]))[-1][:2] == ('ZB', 'Z')
    good = str(tmp_path / 'good.bam')
    shutil.copy(ts.tmp_bam, good)
    with bam_out.BamWriter(ts.tmp_bam, header) as w:
        for i, r in enumerate(recs):
            w.write(r[:-2] if i == k else r)                     # ZB:Z loses its NUL
    with pytest.raises(ValueError, match=re.escape('record %d (%s): a Z / H aux value has no NUL' % (k, bam_out.qname_of(recs[k])))):
        ts.update_sam(tl, o.outfile_path('updated.bam'), command_line='t')
    with bam_out.BamWriter(ts.tmp_bam, header) as w:
        for r in recs[:-1]:
            w.write(r)
    with pytest.raises(ValueError, match='holds %d records, the load wrote %d' % (len(recs) - 1, len(recs))):
        ts.update_sam(tl, o.outfile_path('updated.bam'), command_line='t')
    shutil.copy(good, ts.tmp_bam)
    ts.update_sam(tl, o.outfile_path('updated.bam'), command_line='t')
    assert _n_records(o.outfile_path('updated.bam')) == len(recs)
