"""`--collate device` on the GPU (telescope_amd/csrc/tsem_bam_collate.hip): the kernels against tsem_bam_collate_host on the small
inputs of _collate_reference (bytes, order and the number of names; a failure names the stage), the device loader on reordered BAMs
against the python loader on their reference-collated copies, and the command line end to end.  Sizes above one block of the
device's sort, every alignment of the gather and both of its widths: tests/test_gpu_collate_scale.py (streams of _collate_streams)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import _bam_fuzz as fuzz
import _collate_reference as cr
import _loader_reference as lr
from conftest import ROOT

pytestmark = pytest.mark.gpu
CASES = cr.cases()
HOWS = ('sorted', 'shuffled')
LABELS = list(cr.FIXTURES) + ['fuzz%d' % s for s in cr.FUZZ_SEEDS]


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('collate'))


@functools.lru_cache(maxsize=None)
def _sources(directory):
    return {s[0]: s for s in cr.sources(directory)}


@functools.lru_cache(maxsize=None)
def _files(directory, label, how):
    """(the reordered BAM, its framed records, gtf, barcode tag, the python loader's dict of the reference-collated copy, annotation)"""
    from telescope_amd import loader
    src = _sources(directory)[label]
    p_in, p_ref, recs = cr.reordered_files(directory, src, how)
    ann = loader.Annotation(src[2], 'locus', 'None')
    return p_in, recs, src[2], src[3], loader.load_alignment(p_ref, ann, barcode_tag=src[3]), ann


def _device_equals_host(records, bits, label):
    from telescope_amd import _lib
    data, off = cr.stream_of(records)
    want, want_order, want_names, _ = _lib.bam_collate(data, off, device=None, hash_bits=bits)
    for run in (1, 2):                                       # the same input twice in one process: identical output
        got, order, names, ms = _lib.bam_collate(data, off, device=0, hash_bits=bits)
        where = '%s, hash_bits %d, run %d' % (label, bits, run)
        assert np.array_equal(order, want_order), 'order differs (hash, insert, key or sort): ' + where
        assert names == want_names, 'n_names differs (insert or key): ' + where
        assert got.tobytes() == want.tobytes(), 'order is equal, the bytes differ (gather): ' + where
        assert sorted(ms) == ['d2h', 'gather', 'h2d', 'hash_insert_key', 'sort_scan'] and all(v >= 0 for v in ms.values())


@pytest.mark.parametrize('bits', cr.HASH_BITS)
@pytest.mark.parametrize('label', list(CASES))
def test_device_equals_host_on_the_built_cases(label, bits, gpu_device):
    _device_equals_host(CASES[label], bits, label)


@pytest.mark.parametrize('bits', cr.HASH_BITS)
@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('label', LABELS)
def test_device_equals_host_on_reordered_files(label, how, bits, gpu_device, workdir):
    _device_equals_host(_files(workdir, label, how)[1], bits, '%s-%s' % (label, how))


@pytest.mark.parametrize('label', list(cr.malformed()))
def test_device_refuses_a_malformed_record_by_its_index(label, gpu_device):
    from telescope_amd import _lib
    recs, bad, code = cr.malformed()[label]
    data, off = cr.stream_of(recs)
    with pytest.raises(ValueError) as e:
        _lib.bam_collate(data, off, device=0)
    assert str(e.value) == 'record %d: %s' % (bad, _lib.COLLATE_STATUS[code])


def _load(bam, ann, btag, **kw):
    from telescope_amd import loader, loader_device
    out = loader.load_alignment(bam, ann, barcode_tag=btag, loader='device', device=0, **kw)
    return out, dict(loader_device.LAST_STATS)


@pytest.mark.parametrize('more', [{}, {'inflate': 'device'}, {'chunk_bytes': 4096}], ids=['plain', 'inflate_device', 'chunk_4096'])
@pytest.mark.parametrize('how', HOWS)
@pytest.mark.parametrize('label', LABELS)
def test_loader_parity_on_reordered_bams(label, how, more, gpu_device, workdir):
    p_in, recs, _gtf, btag, want, ann = _files(workdir, label, how)
    kw = dict(more, record_cap=fuzz.RECORD_CAP) if label.startswith('fuzz') else more
    got, stats = _load(p_in, ann, btag, collate='device', **kw)
    lr.assert_same_load(got, want)
    assert stats['collate'] == 'device' and stats['collate_s'] > 0 and set(stats['collate_ms']) == {'h2d', 'hash_insert_key', 'sort_scan', 'gather', 'd2h'}
    assert stats['records'] == len(recs)
    if label.startswith('fuzz'):
        assert stats['fallbacks'] == fuzz.EXPECTED_FALLBACKS
    if more.get('inflate') == 'device':
        assert stats['inflate'] == 'device'


@pytest.mark.parametrize('how', ['host', 'device'])
@pytest.mark.parametrize('name', ['loader_mixed', 'sc_mixed'])
def test_collating_a_collated_fixture_changes_nothing(name, how, gpu_device):
    from telescope_amd import loader
    bam, gtf = lr.fixture_paths(name)
    ann = loader.Annotation(gtf, 'locus', 'None')
    btag = lr.FIXTURES[name][0]
    want, s0 = _load(bam, ann, btag)
    got, s1 = _load(bam, ann, btag, collate=how)
    lr.assert_same_load(got, want)
    assert 'collate' not in s0 and 'collate_s' not in s0 and 'collate_ms' not in s0 and s1['collate'] == how


def test_without_collate_the_sorted_bam_loads_differently(gpu_device, workdir):
    """the inputs exercise the feature: the same reordered files, loaded as they are, give another result"""
    differ = []
    for label in ('loader_mixed', 'sc_mixed', 'fuzz0', 'fuzz1'):
        p_in, _recs, _gtf, btag, want, ann = _files(workdir, label, 'sorted')
        got, stats = _load(p_in, ann, btag, collate='none')
        assert 'collate' not in stats
        try:
            lr.assert_same_load(got, want)
        except AssertionError:
            differ.append(label)
    assert differ == ['loader_mixed', 'sc_mixed', 'fuzz0', 'fuzz1']


# ------------------------------------------------------------------------------------------------------------------ the CLI
def _cli(argv, outdir):
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize('sc', [False, True])
def test_assign_collate_device_writes_the_reports_of_the_collated_bam(sc, gpu_device, workdir, tmp_path):
    label = 'sc_mixed' if sc else 'bundled'
    src = _sources(workdir)[label]
    p_in, p_ref, _recs = cr.reordered_files(str(tmp_path), src, 'sorted')
    head = ['sc'] if sc else []
    _cli(head + ['assign', p_in, src[2], '--loader', 'device', '--collate', 'device'], tmp_path / 'c')
    _cli(head + ['assign', p_ref, src[2], '--loader', 'device'], tmp_path / 'r')
    names = sorted(os.listdir(str(tmp_path / 'c')))
    assert names == sorted(os.listdir(str(tmp_path / 'r'))) and 'telescope-run_stats.tsv' in names
    assert any(n.startswith('telescope-TE_counts') for n in names) and any(n.endswith('.npz') for n in names)
    for n in names:
        if n.endswith('.npz'):                              # (the checkpoint: the same arrays; the zip container carries time stamps)
            with np.load(str(tmp_path / 'c' / n), allow_pickle=True) as x, np.load(str(tmp_path / 'r' / n), allow_pickle=True) as y:
                assert sorted(x.files) == sorted(y.files)
                for k in x.files:
                    assert np.array_equal(x[k], y[k]), k
        else:
            assert open(str(tmp_path / 'c' / n), 'rb').read() == open(str(tmp_path / 'r' / n), 'rb').read(), n
