"""`--deflate device`, `-m gpu`: k_bgzf_deflate is held to tsem_bgzf_deflate_host — the same body with one lane on the CPU — byte for
byte on every case of tests/_bgzf_deflate_reference.py and on batches of mixed blocks; gzip, the header walk and the device inflate read
the result back.  Then bgzf.DeviceBgzfWriter against bam_out.BgzfWriter's cuts, and the command line end to end: the three BAMs of
`--updated_sam --deflate device` inflate to the bytes of the `--deflate host` run of the same route, everything else is the same file."""
import filecmp
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import _bgzf_deflate_reference as dref
import _bgzf_reference as bref
import _loader_reference as lr
from telescope_amd import _lib, bam_out, bgzf, loader

pytestmark = pytest.mark.gpu
BLOCK = dref.BLOCK


@pytest.fixture(scope='module')
def dev(gpu_device):
    d = _lib.BgzfDeflater(gpu_device)
    yield d
    d.close()


@pytest.fixture(scope='module')
def all_cases(tmp_path_factory):
    c = dref.cases().copy()
    c.update(dref.fuzz_cases(str(tmp_path_factory.mktemp('bgzf_deflate_fuzz'))))
    return c


def _check(dev, data, gpu_device, inflate=True):
    image = dev.deflate(data).tobytes()
    assert image == _lib.bgzf_deflate_host(data).tobytes()
    dref.check_image(data, image)
    if data:
        assert gzip.decompress(image) == data
    blocks, used, not_bgzf = _lib.bgzf_scan(image)
    assert used == len(image) and not not_bgzf and len(blocks) == (len(data) + BLOCK - 1) // BLOCK
    if inflate:
        assert bgzf.inflate(image + bam_out.BGZF_EOF, device=gpu_device) == data
    return image, blocks


def test_every_case(dev, all_cases, gpu_device):
    for name, data in all_cases.items():
        try:
            _check(dev, data, gpu_device)
        except AssertionError as e:
            raise AssertionError('case %s: %s' % (name, e))


def _mixed(n, seed):
    """n blocks of mixed cases, the last one short: block k is cut out of one of the cases"""
    c = dref.cases()
    pool = [c[k] for k in ('zeros_65280', 'random_65280', 'period_3', 'period_65', 'period_32768', 'period_40000', 'alphabet16', 'fibonacci_literals',
                           'bam_sc_umi', 'bam_bundled_alignment')]
    rng = np.random.RandomState(seed)
    parts = []
    for k in range(n):
        src = pool[rng.randint(len(pool))]
        at = rng.randint(0, max(1, len(src) - BLOCK))
        parts.append((src[at:at + BLOCK] * (BLOCK // max(1, len(src[at:at + BLOCK])) + 1))[:BLOCK])
    parts[-1] = parts[-1][:int(rng.randint(1, BLOCK))]
    return b''.join(parts)


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 300])
def test_batches_of_mixed_blocks(dev, gpu_device, n):
    """one call, every block at the prefix sum of the sizes in front of it (the header walk finds each where the last one ends)"""
    data = _mixed(n, n)
    image, blocks = _check(dev, data, gpu_device, inflate=n <= 65)
    sizes = [len(p) + 26 for p, _c, _i in dref.split_blocks(image)]
    assert blocks[:, 0].tolist() == (np.cumsum([0] + sizes)[:-1]).tolist()
    assert dev.times()['batches'] >= 1


def _isizes(path):
    return [i for _p, _c, i in dref.split_blocks(open(path, 'rb').read())]


@pytest.mark.parametrize('step', [1, 700, 65281])
def test_device_writer(gpu_device, tmp_path, step):
    stream = bref._alphabet16(2 * BLOCK + 12345, 7)
    pieces = [stream[k:k + step] for k in range(0, len(stream), step)]
    a, b = str(tmp_path / 'device.bgzf'), str(tmp_path / 'host.bgzf')
    with bgzf.DeviceBgzfWriter(a, device=gpu_device, batch_bytes=BLOCK) as w:
        for p in pieces:
            w.write(p)
    assert (w.blocks, w.batches) == (3, 3) and w.times()['batches'] == 3
    with bam_out.BgzfWriter(b) as h:
        for p in pieces:
            h.write(p)
    got = open(a, 'rb').read()
    assert got == bgzf.deflate(stream, device=gpu_device) and got.endswith(bam_out.BGZF_EOF)
    assert _isizes(a) == _isizes(b) == [BLOCK, BLOCK, 12345, 0]
    assert gzip.decompress(got) == stream


def test_device_writer_empty_and_failing(gpu_device, tmp_path):
    a = str(tmp_path / 'empty.bgzf')
    with bgzf.DeviceBgzfWriter(a, device=gpu_device):
        pass
    assert open(a, 'rb').read() == bam_out.BGZF_EOF == bgzf.deflate(b'', device=gpu_device)
    w = bgzf.DeviceBgzfWriter(str(tmp_path / 'broken.bgzf'), device=gpu_device)
    with pytest.raises(TypeError):
        w.write(3)                                           # an exception in the middle: both handles are closed
    assert w._fh is None and w._dev is None
    with pytest.raises(ValueError):
        w.write(b'x')


# ------------------------------------------------------------------------------------------------------------------- end to end
def _cli(args, cwd):
    return subprocess.run([sys.executable, '-m', 'telescope_amd'] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, PYTHONPATH=bref.ROOT + os.pathsep + os.environ.get('PYTHONPATH', '')))


@pytest.mark.parametrize('route', ['python', 'device'])
@pytest.mark.parametrize('name', ['bundled', 'sc_mixed'])
def test_cli_end_to_end(gpu_device, tmp_path, name, route):
    bam, gtf = lr.fixture_paths(name)
    head = ['sc', 'assign', bam, gtf, '--barcode_tag', 'CB'] if name == 'sc_mixed' else ['assign', bam, gtf]
    more = ['--loader', 'device', '--rewrite', 'device'] if route == 'device' else []
    dirs = {}
    for deflate in ('host', 'device'):                       # (each in a directory of its own with the same --outdir: one command line but for the route)
        os.mkdir(str(tmp_path / deflate))
        dirs[deflate] = str(tmp_path / deflate / 'out')
        p = _cli(head + ['--updated_sam', '--outdir', 'out', '--deflate', deflate] + more, str(tmp_path / deflate))
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        if deflate == 'device':
            assert b'--deflate device' in p.stderr and p.stderr.count(b'device deflate: ') == 2, p.stderr.decode()[-3000:]
    names = sorted(os.listdir(dirs['host']))
    assert names == sorted(os.listdir(dirs['device']))
    bams = [f for f in names if f.endswith('.bam')]
    assert sorted(bams) == ['telescope-other.bam', 'telescope-tmp_tele.bam', 'telescope-updated.bam']
    for f in names:
        a, b = os.path.join(dirs['host'], f), os.path.join(dirs['device'], f)
        if f.endswith('.bam'):
            x, y = gzip.open(a).read(), gzip.open(b).read()
            if f == 'telescope-updated.bam':                 # its @PG line quotes the command line, which names the route
                assert y.count(b'--deflate device') == 1
                lx, ly = struct.unpack_from('<i', x, 4)[0], struct.unpack_from('<i', y, 4)[0]
                assert ly == lx + 2 and x[8:8 + lx] == y[8:8 + ly].replace(b'--deflate device', b'--deflate host'), f
                x, y = x[8 + lx:], y[8 + ly:]
            assert x == y, f
            assert open(b, 'rb').read().endswith(bam_out.BGZF_EOF)
        else:
            assert filecmp.cmp(a, b, shallow=False), f
    _refs, segs, _header = loader.read_bam(os.path.join(dirs['device'], 'telescope-updated.bam'), raw=True)
    assert sum(1 for _ in segs) > 0


def test_cli_refuses_without_updated_sam(gpu_device, tmp_path):
    bam, gtf = lr.fixture_paths('loader_mixed')
    out = tmp_path / 'never'
    p = _cli(['assign', bam, gtf, '--deflate', 'device', '--outdir', str(out)], str(tmp_path))
    assert p.returncode != 0 and b'--deflate device without --updated_sam' in p.stderr
    assert not out.exists()
