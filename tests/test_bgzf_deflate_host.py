"""What of the device deflate (`assign --updated_sam --deflate device`) needs no GPU: the body of k_bgzf_deflate — the same functions,
compiled as an ordinary host program under the address and undefined-behaviour sanitizers, with one lane and with 64 lanes run phase by
phase — and tsem_bgzf_deflate_host on every case of tests/_bgzf_deflate_reference.py, both held to zlib and to each other; the
code-length builder on histograms of its own; the Python walker's proof of what the cases exercise; the argument checks of the new
entry points and the command line's refusal.

The sanitized program's run with 64 lanes switches threads 64 times per barrier (0.8 s per block of 65,280 bytes), so of the one long
case, the 267 blocks of bundled_alignment's record stream, that run gets the first four blocks and the end
(_bgzf_deflate_reference.program_input); the program's one-lane run and tsem_bgzf_deflate_host take the stream whole."""
import ctypes as C
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _bgzf_deflate_reference as dref
from _bgzf_reference import ROOT
from telescope_amd import _lib


@pytest.fixture(scope='module')
def workdir(tmp_path_factory):
    return str(tmp_path_factory.mktemp('bgzf_deflate_host'))


@pytest.fixture(scope='module')
def host_program(workdir):
    return dref.build_host_program(workdir)


@pytest.fixture(scope='module')
def all_cases(workdir):
    c = dref.cases().copy()
    c.update(dref.fuzz_cases(workdir))
    return c


@pytest.fixture(scope='module')
def program_images(host_program, all_cases, workdir):
    """name -> (BGZF bytes, rows) of the sanitized program, every case once"""
    names = list(all_cases)
    with ThreadPoolExecutor(max_workers=8) as ex:
        got = list(ex.map(lambda n: dref.host_run(host_program, dref.program_input(n, all_cases[n]), workdir, n), names))
    return dict(zip(names, got))


@pytest.fixture(scope='module')
def long_image(host_program, all_cases, workdir):
    """the whole long record stream through the sanitized program, one lane"""
    return dref.host_run(host_program, all_cases[dref.LONG_CASE], workdir, dref.LONG_CASE + '_whole', mode='blocks1')


@pytest.fixture(scope='module')
def host_images(all_cases):
    return {n: _lib.bgzf_deflate_host(d).tobytes() for n, d in all_cases.items()}


@pytest.fixture(scope='module')
def walked(all_cases, host_images):
    """name -> the walker's blocks of the case's FIRST stream"""
    return {n: dref.walk(dref.split_blocks(host_images[n])[0][0]) for n in all_cases if all_cases[n]}


def test_code_length_builder(host_program):
    lines = dref.lengths_run(host_program)
    assert len(lines) == 21 and all(l.endswith(' ok') for l in lines), lines
    by = {l.split()[0]: l.split() for l in lines}
    assert by['fibonacci_286'][8] == '15' and by['fibonacci_19'][8] == '7'      # the limit is reached: an unlimited code would pass it
    assert by['one_symbol_30'][6] == '1' and by['two_symbols_286'][8] == '1'


def test_program_every_case(all_cases, program_images):
    """one lane and 64 lanes agree and bgzf_inflate_block reads the stream back (the program's own checks); zlib agrees"""
    for n, data in all_cases.items():
        image, rows = program_images[n]
        part = dref.program_input(n, data)
        if not part:
            assert rows == [(0, 2, 1)] and dref.split_blocks(image)[0] == (b'\x03\x00', 0, 0), n      # the empty block: fixed, end-of-block
            continue
        blocks = dref.check_image(part, image)
        assert [r[1] for r in rows] == [len(b[0]) for b in blocks], n


def test_host_entry_every_case(all_cases, host_images, program_images, long_image):
    """tsem_bgzf_deflate_host: the bytes of the program, valid by zlib, never above len + 5"""
    for n, data in all_cases.items():
        image = host_images[n]
        dref.check_image(data, image)
        if not data:
            assert image == b''
        elif n == dref.LONG_CASE:
            got = program_images[n][0]
            k = dref.LONG_HEAD // dref.BLOCK
            head = image[:sum(len(b[0]) + 26 for b in dref.split_blocks(image)[:k])]      # (the excerpt's first blocks are the stream's)
            assert len(head) > 26 * k and got[:len(head)] == head, n
            assert long_image[0] == image and len(long_image[1]) == 267, n
        else:
            assert image == program_images[n][0], n


def test_cut_points(host_images, all_cases):
    assert [b[2] for b in dref.split_blocks(host_images['three_blocks_and_one'])] == [0xff00, 0xff00, 0xff00, 1]
    assert [b[2] for b in dref.split_blocks(host_images['exactly_one_block'])] == [0xff00]
    blocks = dref.split_blocks(host_images['random_65280'])
    assert len(blocks[0][0]) == 0xff00 + 5 and len(host_images['random_65280']) == 65311 < 65536      # stored, LEN = 0xff00


def test_periods(host_images):
    """a unit within the window compresses; one beyond it comes out valid (check_image above) — no distance beyond 32,768"""
    for P in dref.PERIODS:
        n = len(host_images['period_%d' % P])
        if P <= 32768:
            assert n < 0xff00 * 2 // 3, (P, n)


def test_coverage(walked):
    """the cases exercise what they claim"""
    blocks = [(n, b) for n, bs in walked.items() for b in bs]
    assert all(len(bs) == 1 for bs in walked.values())                       # one DEFLATE block per stream
    assert any(b['type'] == 0 for _n, b in blocks) and any(b['type'] == 1 for _n, b in blocks) and any(b['type'] == 2 for _n, b in blocks)
    assert walked['len_1'][0]['type'] == 1 and walked['random_65280'][0]['type'] == 0
    assert any(285 in b['len_syms'] for _n, b in blocks)
    assert any(29 in b['dist_syms'] for _n, b in blocks)
    assert any(b['type'] == 2 and b['n_dist_codes'] == 0 and not b['dist_syms'] for _n, b in blocks)
    assert any(b['type'] == 2 and b['n_dist_codes'] == 1 and b['d_lens'] == {1} for _n, b in blocks)
    assert walked['zeros_65280'][0]['dist_syms'] == {0} and 285 in walked['zeros_65280'][0]['len_syms']
    assert walked['de_bruijn_5_3'][0]['type'] == 2 and walked['de_bruijn_5_3'][0]['n_dist_codes'] == 0
    # the limit of 15 bits at work inside a block: this stream's own histogram wants 18 (and nothing in it was matched away)
    deep = walked['fibonacci_over_flat_literals'][0]
    assert deep['type'] == 2 and not deep['dist_syms'] and sum(deep['ll_hist'].values()) == 200 * 256 + 232
    assert dref.huffman_depth(deep['ll_hist']) == 18 and max(deep['ll_lens']) == 15
    assert all(max(b['ll_lens'] | b['d_lens'] | {0}) <= 15 and max(b['cl_lens'] | {0}) <= 7 for _n, b in blocks)
    assert all(b['spelled_runs'] == 0 for _n, b in blocks)                   # the lengths are spelled out


def test_compresses(all_cases, host_images):
    """guards against a compressor that quietly does nothing; both bounds are derived, not measured"""
    # fixed codes, greedy matches of 258 at distance 1: a literal, 253 matches of 258 + 13 bits each... 412 bytes; the frame is 26
    assert len(host_images['zeros_65280']) - 26 <= 512
    for n, data in all_cases.items():
        if n.startswith('bam_'):
            assert len(host_images[n]) < dref.fixed_literal_cost(data), n


def test_argument_refusals():
    L = _lib.lib()
    n_out, n_blk = C.c_int64(), C.c_int64()
    data = np.zeros(70000, np.uint8)
    out = np.zeros(70000 + 62, np.uint8)
    p = _lib.ptr
    host = lambda *a: L.tsem_bgzf_deflate_host(*a)
    dev = lambda *a: L.tsem_bgzf_deflate(None, *a)           # (a NULL handle: the arguments are checked before it is looked at)
    for f in (host, dev):
        assert f(p(data), -1, p(out), out.size, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG
        assert f(None, 5, p(out), out.size, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG
        assert f(p(data), data.size, p(out), -1, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG
        assert f(p(data), data.size, p(out), out.size - 1, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG      # the worst case: 31 per block
        assert b'31 per block' in L.tsem_last_error(None)
        assert f(p(data), data.size, None, out.size, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG
        assert f(p(data), data.size, p(out), out.size, None, C.byref(n_blk)) == _lib.ERR_ARG
        assert f(p(data), data.size, p(out), out.size, C.byref(n_out), None) == _lib.ERR_ARG
    assert dev(p(data), data.size, p(out), out.size, C.byref(n_out), C.byref(n_blk)) == _lib.ERR_ARG
    assert b'NULL handle' in L.tsem_last_error(None)
    assert host(p(data), data.size, p(out), out.size, C.byref(n_out), C.byref(n_blk)) == _lib.OK and n_blk.value == 2
    assert host(None, 0, None, 0, C.byref(n_out), C.byref(n_blk)) == _lib.OK and (n_out.value, n_blk.value) == (0, 0)
    assert L.tsem_bgzf_deflate_times(None, 0, None, None) == _lib.ERR_ARG
    assert _lib.bgzf_deflate_host(b'').size == 0


def test_writer_and_loaders_refuse_unknown_routes(tmp_path):
    from telescope_amd import bam_out, loader
    with pytest.raises(ValueError, match='deflate'):
        bam_out.BamWriter(str(tmp_path / 'x.bam'), dict(text='', refs_block=b'\x00' * 4), deflate='gpu')
    with pytest.raises(ValueError, match='deflate'):
        loader.load_alignment('none.bam', None, deflate='gpu')
    with pytest.raises(ValueError, match='updated_sam'):
        loader.load_alignment('none.bam', None, deflate='device')
    assert not os.path.exists(str(tmp_path / 'x.bam'))


def test_cli_refuses_device_deflate_without_updated_sam(tmp_path):
    out = tmp_path / 'never'
    for sub in (['assign'], ['sc', 'assign']):
        p = subprocess.run([sys.executable, '-m', 'telescope_amd'] + sub + ['--deflate', 'device', '--outdir', str(out), 'none.bam', 'none.gtf'],
                           cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode != 0 and b'--deflate device without --updated_sam' in p.stderr, p.stderr.decode()[-2000:]
        assert not out.exists()
