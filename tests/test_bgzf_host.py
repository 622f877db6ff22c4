"""What of the device inflate (`assign --loader device --inflate device`) needs no GPU: the header walk tsem_bgzf_scan against a Python
walk of the same bytes, the inflate body of k_bgzf_inflate — the same functions, compiled as an ordinary host program under the address
and undefined-behaviour sanitizers — against zlib on every case of tests/_bgzf_reference.py, the corrupt ones included, the argument
checks of the new entry points, and the command line's refusals."""
import gzip
import os
import zlib

import numpy as np
import pytest

import _bgzf_reference as bref
from conftest import GOLD


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('bgzf_host'))


@pytest.fixture(scope='module')
def host_program(workdir):
    return bref.build_host_program(workdir)


# ------------------------------------------------------------------------------------------------------------ the cases themselves
def test_every_corrupt_status_code_has_a_case():
    assert sorted(set(c.status for c in bref.corrupt_cases())) == list(range(1, 11))
    assert all(c.status == 0 and zlib.crc32(c.expected) == zlib.crc32(zlib.decompress(c.payload, -15)) for c in bref.all_valid())


def test_the_cases_cover_the_block_types_the_issue_names():
    """the first DEFLATE block's type, read from the payload's first three bits, of the cases that are named after one"""
    btype = {c.name: (c.payload[0] >> 1) & 3 for c in bref.all_valid()}
    assert btype['level0_stored'] == 0 and btype['incompressible'] == 0 and btype['fixed'] == 1
    assert all(btype[n] == 2 for n in ('level1', 'level6', 'level9', 'huffman_only', 'rle_equal_bytes', 'long_codes'))
    by = {c.name: c for c in bref.all_valid()}
    assert len(by['rle_equal_bytes'].payload) < 200 and len(by['long_distances'].expected) == 64000
    assert len(by['long_distances'].payload) < 33000         # the second half is matches at distance 32,000


# ------------------------------------------------------------------------------------------------------------------- tsem_bgzf_scan
def _scan(data, cap=None):
    from telescope_amd import _lib
    blk, used, nb = _lib.bgzf_scan(data, cap)
    return blk.tolist(), used, nb


@pytest.mark.parametrize('name', bref.FIXTURE_BAMS)
def test_scan_matches_the_python_walk_on_the_fixtures(name):
    data = open(os.path.join(GOLD, name), 'rb').read()
    rows, used, nb = bref.walk_headers(data)
    assert _scan(data) == (rows, used, nb) and used == len(data) and not nb
    if name == 'bundled_alignment.bam':
        assert len(rows) == 270 and max(r[3] for r in rows) == 65280 and max(r[2] + 26 for r in rows) == 6757   # (whole blocks)
    with gzip.open(os.path.join(GOLD, name), 'rb') as g:     # ... and the walk itself: payloads and trailers are those of the file
        want = g.read()
    got = b''.join(zlib.decompress(data[r[1]:r[1] + r[2]], -15) for r in rows)
    assert got == want and all(zlib.crc32(zlib.decompress(data[r[1]:r[1] + r[2]], -15)) == r[4] for r in rows[:5])


def test_scan_of_the_cases_and_of_a_buffer_cut_at_every_offset():
    cs = [c for c in bref.all_valid() if len(c.payload) < 200] + list(bref.corrupt_cases()[:3])
    front = b'XY\x03\x00abc' + b'ZZ\x00\x00'                 # two other subfields ahead of BC
    blocks = [bref.case_block(c, front if k % 2 else b'') for k, c in enumerate(cs)]
    data = b''.join(blocks)
    rows, used, nb = bref.walk_headers(data)
    assert len(rows) == len(cs) and used == len(data) and not nb
    assert [r[2] for r in rows] == [len(c.payload) for c in cs] and rows[1][1] - rows[1][0] == 12 + len(front) + 6
    assert _scan(data) == (rows, used, nb)
    # cut inside a header, a payload and a trailer: the partial block is not consumed
    ends = np.cumsum([len(b) for b in blocks]).tolist()
    for cut in range(ends[2] + 1):
        whole = sum(1 for e in ends if e <= cut)
        got = _scan(data[:cut])
        assert got == bref.walk_headers(data[:cut]), cut
        assert len(got[0]) == whole and got[1] == ([0] + ends)[whole] and not got[2], cut
    # at most `cap` blocks
    assert _scan(data, cap=2) == (rows[:2], ends[1], False)
    assert _scan(b'') == ([], 0, False)


def test_scan_tells_plain_gzip_and_other_bytes_from_bgzf():
    from telescope_amd import _lib
    plain = gzip.compress(b'BAM\x01' + bytes(100))
    assert plain[3] == 0 and _scan(plain) == ([], 0, True) == bref.walk_headers(plain)
    no_bc = b'\x1f\x8b\x08\x04' + bytes(6) + b'\x06\x00' + b'XY\x02\x00ab' + bref.EOF_PAYLOAD + bytes(8)
    assert _scan(no_bc) == ([], 0, True) == bref.walk_headers(no_bc)
    assert _scan(b'BAM\x01' + bytes(40)) == ([], 0, True)
    good = bref.case_block(bref.zlib_made()[1])
    with pytest.raises(_lib.EngineError) as e:               # behind the first block such bytes cannot be stepped over
        _lib.bgzf_scan(good + plain)
    assert e.value.code == _lib.ERR_ARG and 'block 1 at byte %d' % len(good) in str(e.value)
    with pytest.raises(_lib.EngineError) as e:
        _lib.bgzf_scan(good + no_bc)
    assert 'no BC subfield' in str(e.value)
    small = bytearray(good)
    small[16:18] = (20).to_bytes(2, 'little')                # BSIZE below header + trailer
    with pytest.raises(_lib.EngineError) as e:
        _lib.bgzf_scan(good + bytes(small))
    assert 'BSIZE' in str(e.value)


# -------------------------------------------------------------------------------------------- the inflate body, sanitized, on the host
@pytest.mark.parametrize('case', bref.all_valid(), ids=lambda c: c.name)
def test_inflate_body_equals_zlib(case, host_program, workdir):
    scan, st, ranges = bref.host_run(host_program, bref.case_block(case), workdir, case.name)
    assert scan[0] == 1 and st == [0]
    assert ranges[0] == case.expected


@pytest.mark.parametrize('case', bref.corrupt_cases(), ids=lambda c: c.name)
def test_inflate_body_stops_a_corrupt_block_with_its_status(case, host_program, workdir):
    data, cs, k = bref.corrupt_batch(case)
    scan, st, ranges = bref.host_run(host_program, data, workdir, case.name)
    assert scan == (len(cs), len(data), 0)
    assert st == [0, 0, case.status, 0, 0]
    for i, c in enumerate(cs):                               # the valid blocks around it come out right
        if i != k:
            assert ranges[i] == c.expected, i


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 300])
def test_inflate_body_on_batches(n, host_program, workdir):
    data, expected, blocks = bref.batch(n)
    scan, st, ranges = bref.host_run(host_program, data, workdir, 'batch%d' % n)
    assert scan == (n, len(data), 0) and st == [0] * n
    assert b''.join(ranges) == expected
    assert n < 3 or any(len(r) == 0 for r in ranges)        # empty blocks among them


def test_inflate_body_on_the_fixtures_and_the_oversize_claim(host_program, workdir):
    for name in bref.FIXTURE_BAMS:
        data = open(os.path.join(GOLD, name), 'rb').read()
        scan, st, ranges = bref.host_run(host_program, data, workdir, name)
        with gzip.open(os.path.join(GOLD, name), 'rb') as g:
            assert b''.join(ranges) == g.read() and not any(st)
    c = bref.oversize_case()
    scan, st, ranges = bref.host_run(host_program, bref.case_block(c), workdir, c.name)
    assert st == [bref.ST_HOST] and ranges == [b'']


# ------------------------------------------------------------------------------------------------ argument checks without a device
def test_argument_checks_of_the_entry_points():
    import ctypes as C
    from telescope_amd import _lib
    L = _lib.lib()
    n, used, nb = C.c_int64(), C.c_int64(), C.c_int32()
    buf = np.frombuffer(bref.case_block(bref.zlib_made()[1]), np.uint8)
    blk = np.zeros((4, 5), np.int64)
    err = lambda: L.tsem_last_error(None).decode()
    assert L.tsem_bgzf_scan(None, 5, _lib.ptr(blk), 4, C.byref(n), C.byref(used), C.byref(nb)) == _lib.ERR_ARG and 'tsem_bgzf_scan' in err()
    assert L.tsem_bgzf_scan(_lib.ptr(buf), -1, _lib.ptr(blk), 4, C.byref(n), C.byref(used), C.byref(nb)) == _lib.ERR_ARG
    assert L.tsem_bgzf_scan(_lib.ptr(buf), buf.size, None, 4, C.byref(n), C.byref(used), C.byref(nb)) == _lib.ERR_ARG
    assert L.tsem_bgzf_scan(_lib.ptr(buf), buf.size, _lib.ptr(blk), 4, None, C.byref(used), C.byref(nb)) == _lib.ERR_ARG
    assert L.tsem_bgzf_scan(_lib.ptr(buf), buf.size, _lib.ptr(blk), 4, C.byref(n), C.byref(used), C.byref(nb)) == _lib.OK and n.value == 1
    assert L.tsem_bgzf_open(None, 0) == _lib.ERR_ARG and 'out is NULL' in err()
    assert L.tsem_bgzf_close(None) == _lib.OK
    ms = np.zeros(3)
    assert L.tsem_bgzf_times(None, 0, _lib.ptr(ms), C.byref(n)) == _lib.ERR_ARG and 'tsem_bgzf_times' in err()
    # tsem_bgzf_inflate checks the table before it looks at the handle: nothing here touches a device
    out, st, first, total = np.zeros(64, np.uint8), np.zeros(4, np.int32), np.zeros(2, np.int64), C.c_int64()
    call = lambda b=buf, nbytes=buf.size, t=blk, nblk=1, o=out, cap=64, s=st, f=first: L.tsem_bgzf_inflate(
        None, None if b is None else _lib.ptr(b), nbytes, None if t is None else _lib.ptr(t), nblk, None if o is None else _lib.ptr(o), cap,
        None if s is None else _lib.ptr(s), None if f is None else _lib.ptr(f), C.byref(total))
    row = blk[0]
    row[:] = [0, 18, buf.size - 26, 1, 0]
    assert call() == _lib.ERR_ARG and 'NULL handle' in err()                      # (a table that passes)
    for kw in (dict(b=None), dict(t=None), dict(s=None), dict(f=None), dict(o=None), dict(nbytes=-1), dict(nblk=-1), dict(cap=-1)):
        assert call(**kw) == _lib.ERR_ARG and 'NULL pointer, negative size' in err(), kw
    for bad in ([0, -1, 3, 1, 0], [0, 18, buf.size, 1, 0], [0, buf.size, 1, 1, 0], [0, 18, -2, 1, 0], [0, 0, 65537, 1, 0]):
        row[:] = bad
        assert call() == _lib.ERR_ARG and 'payload of block 0 lies outside the bytes' in err(), bad
    row[:] = [0, 18, 3, 1 << 32, 0]
    assert call() == _lib.ERR_ARG and 'no 32-bit value' in err()
    row[:] = [0, 18, 3, 65, 0]
    assert call() == _lib.ERR_ARG and 'inflate to 65 bytes, out holds 64' in err()
    blk[:2] = [[0, 18, 3, 40, 0], [0, 18, 3, 40, 0]]
    assert call(nblk=2) == _lib.ERR_ARG and 'inflate to 80 bytes' in err()
    blk[1, 3] = 70000                                        # a claim above 64 KiB takes no room: the table passes
    assert call(nblk=2) == _lib.ERR_ARG and 'NULL handle' in err()
    assert sorted(_lib.BGZF_STATUS) == list(range(1, 11))


# --------------------------------------------------------------------------------------------------------------- the command line
def test_cli_takes_the_inflate_option_and_refuses_it_without_the_device_loader(tmp_path, capsys):
    from telescope_amd import cli
    ap = cli.build_parser()
    for argv in (['assign', 'a.bam', 'a.gtf'], ['sc', 'assign', 'a.bam', 'a.gtf']):
        assert ap.parse_args(argv).inflate == 'host'
        assert ap.parse_args(argv + ['--loader', 'device', '--inflate', 'device']).inflate == 'device'
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ['--inflate', 'zlib'])
        for extra in ([], ['--loader', 'python']):           # before anything is read: the files do not exist
            with pytest.raises(SystemExit) as e:
                cli.main(argv[:-2] + [str(tmp_path / 'none.bam'), str(tmp_path / 'none.gtf'), '--inflate', 'device', '--outdir',
                                      str(tmp_path / 'o')] + extra)
            assert '--inflate device without --loader device is not supported' in str(e.value)
            assert not os.path.exists(str(tmp_path / 'o'))
    capsys.readouterr()


def test_inflate_keyword_is_checked():
    from telescope_amd import loader
    bam, gtf = os.path.join(GOLD, 'loader_mixed.bam'), os.path.join(GOLD, 'loader_mixed.gtf')
    ann = loader.Annotation(gtf, 'locus', 'None')
    with pytest.raises(ValueError):
        loader.load_alignment(bam, ann, inflate='device')                        # needs loader='device'
    with pytest.raises(ValueError):
        loader.load_alignment(bam, ann, loader='device', inflate='zlib')
    want = loader.load_alignment(bam, ann)
    got = loader.load_alignment(bam, ann, inflate='host')
    assert np.array_equal(got['raw_scores'].data, want['raw_scores'].data)
