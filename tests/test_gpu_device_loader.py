"""The device loader (`load_alignment(loader='device')`, telescope_amd/loader_device.py + csrc/tsem_bam.hip) against the Python loader:
the whole dict on the fixtures and on seeded fuzz cases, the raw outputs of every kernel against the stage reference, chunk sizes
that force carried bundles and growing chunks, malformed records in the middle of a chunk, and the command line end to end."""
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import _bam_fuzz as fuzz
import _loader_reference as lref
from _loader_reference import FIXTURES, fixture_paths
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
MODES = ['None', 'F', 'R', 'FR', 'RF']


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('device_loader'))


@functools.lru_cache(maxsize=None)
def _fuzz_reference(seed, directory):
    """(case, stage reference, annotation) of one fuzz case, computed once; the stranded mode goes round with the seed"""
    c = fuzz.make_case(seed, directory)
    ref, ann = lref.reference(c.bam, c.gtf, MODES[seed % 5], 'CB', 'UB')
    return c, ref, ann


@functools.lru_cache(maxsize=None)
def _python_load(name, mode):
    from telescope_amd import loader
    bam, gtf = fixture_paths(name)
    btag, utag = FIXTURES[name]
    ann = loader.Annotation(gtf, 'locus', mode)
    return loader.load_alignment(bam, ann, stranded_mode=mode, barcode_tag=btag, umi_tag=utag), ann


def _device_load(bam, ann, mode, btag, utag, **kw):
    from telescope_amd import loader, loader_device
    out = loader.load_alignment(bam, ann, stranded_mode=mode, barcode_tag=btag, umi_tag=utag, loader='device', device=0, **kw)
    return out, dict(loader_device.LAST_STATS)


@pytest.mark.parametrize('name,mode', [('loader_mixed', m) for m in MODES] + [(n, 'None') for n in ('sc_mixed', 'sc_umi', 'updated_mixed', 'bundled')])
def test_fixture_parity_without_fallbacks(name, mode, gpu_device):
    want, ann = _python_load(name, mode)
    got, stats = _device_load(fixture_paths(name)[0], ann, mode, *FIXTURES[name])
    lref.assert_same_load(got, want)
    assert stats['fallbacks'] == 0                          # (the fallback must not hide a kernel that is wrong on ordinary input)
    if name == 'loader_mixed':                              # ... and the fixture the reference program itself produced
        exp = np.load(os.path.join(GOLD, 'loader_mixed_expected.npz'), allow_pickle=False)
        g = lambda k: exp['%s_%s' % (mode, k)]
        raw = got['raw_scores'].tocsr().copy()
        raw.sort_indices()
        assert np.array_equal(raw.indptr, g('indptr')) and np.array_equal(raw.indices, g('indices')) and np.array_equal(raw.data, g('data'))
        assert list(got['read_index']) == list(g('rows')) and list(got['feat_index']) == list(g('cols'))
        assert [int(v) for v in got['run_info'].values()] == g('info').tolist()


@pytest.mark.parametrize('seed', range(20))
def test_fuzz_parity_with_exactly_the_built_fallbacks(seed, gpu_device, workdir):
    c, ref, ann = _fuzz_reference(seed, workdir)
    got, stats = _device_load(c.bam, ann, MODES[seed % 5], 'CB', 'UB', record_cap=fuzz.RECORD_CAP)
    lref.assert_same_load(got, ref.result)
    assert stats['fallbacks'] == c.expected_fallbacks and stats['records'] == c.n_records


@pytest.mark.parametrize('seed', range(20))
def test_stage_parity_names_the_kernel(seed, gpu_device, workdir):
    from telescope_amd import loader_device as ld
    c, ref, ann = _fuzz_reference(seed, workdir)
    mode = MODES[seed % 5]
    chunks = []
    ld.load_alignment_device(c.bam, ann, stranded_mode=mode, barcode_tag='CB', umi_tag='UB', record_cap=fuzz.RECORD_CAP,
                             on_chunk=lambda data, off, out: chunks.append(out.copy()))
    base, parts = 0, []
    for out in chunks:                                      # record indices of a chunk -> of the file
        out = out.copy()
        for col in (ld.C_PAIR1, ld.C_PAIR2, ld.C_BUNDLE):
            out[col][out[col] >= 0] += base
        parts.append(out)
        base += out.shape[1]
    mat = np.concatenate(parts, axis=1)
    over_cap = [b['first'] for b in ref.bundles if b['n'] > fuzz.RECORD_CAP]
    hosted = np.flatnonzero(mat[ld.C_BCLASS] == ld.CLS_HOST).tolist()
    assert len(over_cap) == 1 and set(over_cap) <= set(hosted) and len(hosted) == c.expected_fallbacks
    lref.compare_stages(ref, ann, mat, host_expected=hosted)


@pytest.mark.parametrize('how', ['chunk_bytes_4096', 'chunk_bytes_64', 'one_bundle_per_chunk'])
def test_chunking_does_not_change_the_load(how, gpu_device, workdir):
    from telescope_amd import loader_device as ld
    cases = [(c.bam, ann, MODES[s % 5], 'CB', 'UB', ref.result, fuzz.RECORD_CAP) for s in (0, 1, 7)
             for c, ref, ann in [_fuzz_reference(s, workdir)]]
    for name in ('loader_mixed', 'sc_umi'):
        want, ann = _python_load(name, 'None')
        cases.append((fixture_paths(name)[0], ann, 'None') + FIXTURES[name] + (want, 4096))
    for bam, ann, mode, btag, utag, want, cap in cases:
        kw = dict(chunk_bytes=4096) if how == 'chunk_bytes_4096' else dict(chunk_bytes=64) if how == 'chunk_bytes_64' else dict(max_bundles=1)
        got = ld.load_alignment_device(bam, ann, stranded_mode=mode, barcode_tag=btag, umi_tag=utag, record_cap=cap, **kw)
        lref.assert_same_load(got, want)
        stats = ld.LAST_STATS
        n_bundles = stats['bundles']
        if how == 'one_bundle_per_chunk':
            assert stats['chunks'] == n_bundles
        else:
            assert stats['chunks'] > 2                      # many chunks: bundles were carried over (4096) or the chunk grew (64)


def _malformed_bam(workdir, kind):
    """fuzz case 0 with one damaged record in the MIDDLE of the stream: valid records lie behind it, so a walk that does not stop at the
    record's end finds bytes to go on with (a NUL, a plausible count) and gives a wrong answer or no error — never a stray access"""
    from telescope_amd.bam_out import BamWriter
    from telescope_amd import loader
    c = fuzz.make_case(0, workdir)
    _refs, records, header = loader.read_bam(c.bam, raw=True)
    recs = [s.raw for s in records]
    k = len(recs) // 2
    r = recs[k]
    name = r[32:32 + r[8] - 1].decode()
    if kind == 'z_without_nul':
        r = r + b'XZZnonul'
    elif kind == 'b_array_past_record':
        r = r + b'XBBS' + struct.pack('<i', 1000) + b'\x01\x00'
    else:                                                   # n_cigar past the record
        r = r[:12] + struct.pack('<H', 60000) + r[14:]
    recs[k] = r
    path = os.path.join(workdir, 'malformed_%s.bam' % kind)
    with BamWriter(path, header) as w:
        for x in recs:
            w.write(x)
    return path, c.gtf, k, name


@pytest.mark.parametrize('kind,text', [('z_without_nul', 'no NUL inside the record'), ('b_array_past_record', 'B aux array runs past the record'),
                                       ('n_cigar_past_record', 'n_cigar runs past the record')])
def test_malformed_record_in_mid_chunk_is_a_value_error_that_names_it(kind, text, gpu_device, workdir):
    from telescope_amd import loader
    bam, gtf, k, name = _malformed_bam(workdir, kind)
    ann = loader.Annotation(gtf, 'locus', 'None')
    with pytest.raises(ValueError) as e:
        loader.load_alignment(bam, ann, loader='device')
    assert text in str(e.value) and 'record %d (%s)' % (k, name) in str(e.value)
    with pytest.raises(ValueError) as e:                    # ... whichever chunk it falls into
        loader.load_alignment(bam, ann, loader='device', chunk_bytes=4096)
    assert text in str(e.value) and 'record %d (%s)' % (k, name) in str(e.value)


def test_mapped_record_without_as_is_a_value_error(gpu_device, workdir):
    from telescope_amd import loader
    from telescope_amd.bam_out import BamWriter
    c = fuzz.make_case(0, workdir)
    _refs, records, header = loader.read_bam(c.bam, raw=True)
    recs = [s.raw for s in records]
    path = os.path.join(workdir, 'no_as.bam')
    with BamWriter(path, header) as w:
        for i, x in enumerate(recs):
            w.write(fuzz.encode('noas', 0, 0, 1100, [(50, 'M')]) if i == 40 else x)
    ann = loader.Annotation(c.gtf, 'locus', 'None')
    with pytest.raises(TypeError):
        loader.load_alignment(path, ann)
    with pytest.raises(ValueError) as e:
        loader.load_alignment(path, ann, loader='device')
    assert 'record 40 (noas)' in str(e.value) and 'no AS tag' in str(e.value)


def _cli(argv, outdir):
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize('sc', [False, True])
def test_assign_writes_the_same_reports_with_either_loader(sc, gpu_device, tmp_path):
    bam, gtf = fixture_paths('sc_mixed' if sc else 'bundled')
    argv = (['sc'] if sc else []) + ['assign', bam, gtf]
    _cli(argv + ['--loader', 'python'], tmp_path / 'p')
    _cli(argv + ['--loader', 'device'], tmp_path / 'd')
    names = sorted(os.listdir(str(tmp_path / 'p')))
    assert names == sorted(os.listdir(str(tmp_path / 'd'))) and 'telescope-run_stats.tsv' in names
    assert any(n.startswith('telescope-TE_counts') for n in names)
    for n in names:
        a, b = open(str(tmp_path / 'p' / n), 'rb').read(), open(str(tmp_path / 'd' / n), 'rb').read()
        if n.endswith('.npz'):                              # (the checkpoint: the same arrays; the zip container carries time stamps)
            with np.load(str(tmp_path / 'p' / n), allow_pickle=True) as x, np.load(str(tmp_path / 'd' / n), allow_pickle=True) as y:
                assert sorted(x.files) == sorted(y.files)
                for k in x.files:
                    assert np.array_equal(x[k], y[k]), k
        else:
            assert a == b, n
