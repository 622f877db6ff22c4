"""The device inflate (telescope_amd/bgzf.py + csrc/tsem_bgzf.hip: k_bgzf_inflate, one wave per BGZF block) against zlib, byte for byte: every
case and batch of tests/_bgzf_reference.py, the status words of the corrupt ones, DeviceBgzfReader against gzip on the fixture BAMs with
pieces that cut blocks and hold less than one, the device loader with `inflate='device'` against the Python loader, and the command line."""
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import _bam_fuzz as fuzz
import _bgzf_reference as bref
import _loader_reference as lref
from _loader_reference import FIXTURES, fixture_paths
from conftest import GOLD, ROOT

pytestmark = pytest.mark.gpu
MODES = ['None', 'F', 'R', 'FR', 'RF']


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('bgzf_inflate'))


@functools.lru_cache(maxsize=None)
def _gunzip(path):
    with gzip.open(path, 'rb') as g:
        return g.read()


# ------------------------------------------------------------------------------------------------------------------ bgzf.inflate
@pytest.mark.parametrize('case', bref.all_valid(), ids=lambda c: c.name)
def test_inflate_equals_zlib(case, gpu_device):
    from telescope_amd import bgzf
    assert bgzf.inflate(bref.case_block(case)) == case.expected
    assert bgzf.inflate(bref.case_block(case, b'XY\x01\x00q')) == case.expected     # another subfield ahead of BC


def test_all_cases_in_one_call(gpu_device):
    from telescope_amd import bgzf
    cs = bref.all_valid()
    assert bgzf.inflate(b''.join(bref.case_block(c) for c in cs)) == b''.join(c.expected for c in cs)


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 300])
def test_batches(n, gpu_device):
    from telescope_amd import bgzf
    data, expected, _blocks = bref.batch(n)
    assert bgzf.inflate(data) == expected


@pytest.mark.parametrize('case', bref.corrupt_cases(), ids=lambda c: c.name)
def test_corrupt_block_in_mid_batch(case, gpu_device):
    from telescope_amd import _lib, bgzf
    data, cs, k = bref.corrupt_batch(case)
    blocks, used, nb = _lib.bgzf_scan(data)
    assert used == len(data) and not nb and len(blocks) == len(cs)
    dev = _lib.BgzfInflater(0)
    try:
        out, st, first = dev.inflate(data, blocks)
    finally:
        dev.close()
    assert st.tolist() == [0, 0, case.status, 0, 0] and first == (case.status, k)
    o = 0
    for i, c in enumerate(cs):                               # the valid blocks of the batch come out right
        n = int(blocks[i, 3])
        if i != k:
            assert out[o:o + n].tobytes() == c.expected, i
        o += n
    with pytest.raises(ValueError) as e:
        bgzf.inflate(data)
    assert 'BGZF block %d at byte %d: %s' % (k, int(blocks[k, 0]), _lib.BGZF_STATUS[case.status]) in str(e.value)


def test_first_failure_is_the_first_in_file_order(gpu_device):
    from telescope_amd import _lib
    cc = bref.corrupt_cases()
    v = bref.zlib_made()
    cs = [v[1], cc[-1], v[5], cc[0], cc[5], v[0]]
    data = b''.join(bref.case_block(c) for c in cs)
    blocks = _lib.bgzf_scan(data)[0]
    dev = _lib.BgzfInflater(0)
    try:
        for _ in range(2):                                   # (the handle's buffers are kept and reused)
            _out, st, first = dev.inflate(data, blocks)
            assert st.tolist() == [c.status for c in cs] and first == (cc[-1].status, 1)
        assert dev.times()['batches'] == 2
    finally:
        dev.close()


def test_a_claim_above_64k_is_left_to_zlib_and_truncation_is_an_error(gpu_device, workdir):
    from telescope_amd import bgzf
    big, v = bref.oversize_case(), bref.zlib_made()
    cs = [v[1], big, v[5], big, v[0]]
    data = b''.join(bref.case_block(c) for c in cs)
    assert bgzf.inflate(data) == b''.join(c.expected for c in cs)
    path = os.path.join(workdir, 'oversize.gz')
    with open(path, 'wb') as fh:
        fh.write(data)
    with bgzf.DeviceBgzfReader(path) as r:
        assert r.read() == b''.join(c.expected for c in cs) and r.fallbacks == 2 and r.inflate == 'device' and r.blocks == 5
    for cut in (len(data) - 1, len(data) - 30, 10):
        with open(path, 'wb') as fh:
            fh.write(data[:cut])
        with pytest.raises(ValueError) as e:
            with bgzf.DeviceBgzfReader(path) as r:
                r.read()
        assert str(e.value).endswith('truncated BGZF block') and path in str(e.value)
        with pytest.raises(ValueError) as e:
            bgzf.inflate(data[:cut])
        assert 'truncated BGZF block' in str(e.value)
    with pytest.raises(ValueError):
        bgzf.inflate(gzip.compress(b'plain'))


# --------------------------------------------------------------------------------------------------------------- DeviceBgzfReader
@pytest.mark.parametrize('batch_bytes', [1, 700, 64 << 10])
@pytest.mark.parametrize('name', bref.FIXTURE_BAMS)
def test_reader_equals_gzip(name, batch_bytes, gpu_device):
    """read sizes 1, 4, 65,537 and everything at once; the small read sizes go through the first 6,000 bytes (more than a whole fixture
    for the smallest, several pieces of 700 bytes for all) and the rest follows in one read"""
    from telescope_amd import bgzf
    path = os.path.join(GOLD, name)
    want = _gunzip(path)
    for size in (1, 4, 65537, -1):
        with bgzf.DeviceBgzfReader(path, batch_bytes=batch_bytes) as r:
            parts, got = [], 0
            if size in (1, 4):
                while got < 6000:
                    b = r.read(size)
                    if not b:
                        break
                    got += len(b)
                    assert len(b) == size or got == len(want)
                    parts.append(b)
                parts.append(r.read())
            elif size > 0:
                while True:
                    b = r.read(size)
                    if not b:
                        break
                    parts.append(b)
                assert all(len(b) == size for b in parts[:-1])
            else:
                parts.append(r.read())
            assert r.read(10) == b'' and r.read() == b''
            assert b''.join(parts) == want, size
            assert r.fallbacks == 0 and r.inflate == 'device'
            if batch_bytes == 700 and len(want) > 100000:
                assert r.batches > 20                        # blocks straddled the pieces
        with pytest.raises(ValueError):
            r.read(1)                                        # closed


def test_reader_reads_plain_gzip_on_the_host(gpu_device, workdir, caplog):
    import logging
    from telescope_amd import bgzf
    path = os.path.join(workdir, 'plain.bam')
    want = _gunzip(os.path.join(GOLD, 'loader_mixed.bam'))
    with open(path, 'wb') as fh:
        fh.write(gzip.compress(want))
    with caplog.at_level(logging.INFO):
        with bgzf.DeviceBgzfReader(path) as r:
            assert r.inflate == 'host' and r.read(4) == b'BAM\x01' and r.read() == want[4:]
    assert sum('is not BGZF' in m for m in caplog.messages) == 1


# ------------------------------------------------------------------------------------------------------------------- the loader
@functools.lru_cache(maxsize=None)
def _python_load(name):
    from telescope_amd import loader
    bam, gtf = fixture_paths(name)
    btag, utag = FIXTURES[name]
    ann = loader.Annotation(gtf, 'locus', 'None')
    return loader.load_alignment(bam, ann, barcode_tag=btag, umi_tag=utag), ann


def _device_load(bam, ann, mode, btag, utag, **kw):
    from telescope_amd import loader, loader_device
    out = loader.load_alignment(bam, ann, stranded_mode=mode, barcode_tag=btag, umi_tag=utag, loader='device', inflate='device', device=0, **kw)
    return out, dict(loader_device.LAST_STATS)


@pytest.mark.parametrize('name', sorted(FIXTURES))
def test_fixture_load_with_the_device_inflate(name, gpu_device):
    want, ann = _python_load(name)
    got, stats = _device_load(fixture_paths(name)[0], ann, 'None', *FIXTURES[name])
    lref.assert_same_load(got, want)
    assert stats['inflate'] == 'device' and stats['inflate_fallbacks'] == 0 and stats['fallbacks'] == 0
    assert stats['inflate_blocks'] == len(bref.walk_headers(open(fixture_paths(name)[0], 'rb').read())[0])
    assert stats['inflate_ms']['batches'] >= 1


@pytest.mark.parametrize('seed', range(5))
def test_fuzz_load_with_the_device_inflate(seed, gpu_device, workdir):
    c = fuzz.make_case(seed, workdir)
    ref, ann = lref.reference(c.bam, c.gtf, MODES[seed % 5], 'CB', 'UB')
    got, stats = _device_load(c.bam, ann, MODES[seed % 5], 'CB', 'UB', record_cap=fuzz.RECORD_CAP)
    lref.assert_same_load(got, ref.result)
    assert stats['inflate'] == 'device' and stats['inflate_fallbacks'] == 0
    assert stats['fallbacks'] == c.expected_fallbacks and stats['records'] == c.n_records


def test_a_fixture_recompressed_with_plain_gzip_loads_the_same_on_the_host_path(gpu_device, workdir):
    want, ann = _python_load('sc_umi')
    path = os.path.join(workdir, 'sc_umi_plain_gzip.bam')
    with open(path, 'wb') as fh:
        fh.write(gzip.compress(_gunzip(fixture_paths('sc_umi')[0])))
    got, stats = _device_load(path, ann, 'None', *FIXTURES['sc_umi'])
    lref.assert_same_load(got, want)
    assert stats['inflate'] == 'host' and stats['inflate_fallbacks'] == 0


def test_a_corrupt_block_in_a_bam_is_a_value_error_that_names_it(gpu_device, workdir):
    from telescope_amd import _lib, loader
    bam, gtf = fixture_paths('bundled')
    data = bytearray(open(bam, 'rb').read())
    rows = bref.walk_headers(bytes(data))[0]
    k = 100
    data[rows[k][1] + rows[k][2]] ^= 0x40                   # the CRC-32 of block 100: behind its payload
    path = os.path.join(workdir, 'bad_crc.bam')
    with open(path, 'wb') as fh:
        fh.write(bytes(data))
    ann = loader.Annotation(gtf, 'locus', 'None')
    with pytest.raises(ValueError) as e:
        loader.load_alignment(path, ann, loader='device', inflate='device')
    assert '%s: BGZF block %d at byte %d: %s' % (path, k, rows[k][0], _lib.BGZF_STATUS[10]) in str(e.value)


# --------------------------------------------------------------------------------------------------------------- the command line
def _cli(argv, outdir):
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir), '--quiet'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]


def test_assign_writes_the_same_checkpoint_and_reports_with_the_device_inflate(gpu_device, tmp_path):
    bam, gtf = fixture_paths('loader_mixed')
    _cli(['assign', bam, gtf, '--loader', 'device'], tmp_path / 'h')
    _cli(['assign', bam, gtf, '--loader', 'device', '--inflate', 'device'], tmp_path / 'd')
    names = sorted(os.listdir(str(tmp_path / 'h')))
    assert names == sorted(os.listdir(str(tmp_path / 'd'))) and 'telescope-run_stats.tsv' in names
    assert any(n.startswith('telescope-TE_counts') for n in names) and any(n.endswith('.npz') for n in names)
    for n in names:
        if n.endswith('.npz'):                               # (the checkpoint: the same arrays; the zip container carries time stamps)
            with np.load(str(tmp_path / 'h' / n), allow_pickle=True) as x, np.load(str(tmp_path / 'd' / n), allow_pickle=True) as y:
                assert sorted(x.files) == sorted(y.files)
                for k in x.files:
                    assert np.array_equal(x[k], y[k]), k
        else:
            assert open(str(tmp_path / 'h' / n), 'rb').read() == open(str(tmp_path / 'd' / n), 'rb').read(), n
