"""The cases and the checks of the BGZF deflate tests (telescope_amd/bgzf.py, csrc/tsem_bgzf.hip, csrc/tsem_bgzf_deflate.h).  zlib is the
arbiter of validity, as it is for the inflate unit: a stream is right when zlib.decompress(payload, -15) gives the input back and it
is no longer than len + 5.  `walk` is a small Python reading of a DEFLATE stream that says which block types, length symbols, distance
symbols and code lengths a stream uses, so that the suite can prove that it exercised what it claims.  `build_host_program` /
`host_run`: the deflate body as a stand-alone host program under the address and undefined-behaviour sanitizers
(tests/c_host/bgzf_deflate_check.cc)."""
import functools
import gzip
import os
import struct
import subprocess
import zlib
from collections import OrderedDict

import numpy as np

import _bam_fuzz
import _bgzf_reference as bref
from _bgzf_reference import CL_ORDER, CSRC, DIST_BASE, DIST_EXTRA, GOLD, LEN_BASE, LEN_EXTRA, ROOT

BLOCK = 0xff00
TILE = 64                                # BGZF_DEF_TILE: the matcher's step
PERIODS = (1, 2, 3, 4, 63, 64, 65, 257, 258, 259, 32767, 32768, 32769, 40000)
FUZZ_SEEDS = (1, 2, 3, 4, 5)
# the 267-block record stream: the sanitized program runs all of it with one lane; the run with 64 lanes, which takes 64 thread switches
# per barrier (0.8 s per block), gets its first blocks and its end
LONG_CASE, LONG_HEAD, LONG_TAIL = 'bam_bundled_alignment', 4 * BLOCK, BLOCK + 4321


def check_stream(data, payload):
    assert zlib.decompress(payload, -15) == data
    assert len(payload) <= len(data) + 5, (len(payload), len(data))


def split_blocks(image):
    """[(payload, CRC-32, ISIZE)] of a BGZF byte string whose headers are the 18 bytes this project writes"""
    out, p = [], 0
    while p < len(image):
        assert image[p:p + 16] == b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00', 'block header at %d' % p
        bsize = struct.unpack_from('<H', image, p + 16)[0] + 1
        crc, isize = struct.unpack_from('<II', image, p + bsize - 8)
        out.append((image[p + 18:p + bsize - 8], crc, isize))
        p += bsize
    assert p == len(image)
    return out


def check_image(data, image):
    """a BGZF byte string without EOF block against its input: the cuts, every stream, CRC-32 and ISIZE, BSIZE below 64 KiB"""
    blocks = split_blocks(image)
    assert len(blocks) == (len(data) + BLOCK - 1) // BLOCK
    for k, (payload, crc, isize) in enumerate(blocks):
        part = data[k * BLOCK:(k + 1) * BLOCK]
        check_stream(part, payload)
        assert isize == len(part) and crc == zlib.crc32(part) and len(payload) + 26 <= 65536
    return blocks


# ----------------------------------------------------------------------------------------------------------------------- the cases
def _period(rng, P, total=BLOCK):
    unit = rng.randint(0, 256, P).astype(np.uint8).tobytes()
    return (unit * (total // P + 1))[:total]


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _fibonacci():
    """byte k appears fib(k) times, k = 1 .. 22 (1, 1, 2, ... 17,711): 46,367 bytes, one block"""
    out = []
    for k, n in enumerate(_fib(22)):
        out += [k + 65] * n
    a = np.array(out, np.uint8)
    np.random.RandomState(23).shuffle(a)
    return a.tobytes()


FLAT_SYMBOLS, FLAT_EACH, RARE_SYMBOLS = 200, 256, 10


def _fibonacci_over_flat():
    """A literal/length histogram that needs 18 bits whatever the matcher does, because there is nothing to match: no word of three
    bytes occurs twice.  Bytes 0 .. 199 occur 256 times each, bytes 200 .. 209 occur 1, 2, 3, 5, ... 89 times — with the one
    end-of-block the Fibonacci counts 1, 1, 2, ... 89, 232 in all, less than one byte of the pool.  An unlimited Huffman code pairs
    that chain of ten levels with a byte of the pool, eight levels down among 201 equal weights: 18 bits for the rarest."""
    rng = np.random.RandomState(1597)
    a = np.concatenate([np.repeat(np.arange(FLAT_SYMBOLS), FLAT_EACH)] +
                       [np.full(n, FLAT_SYMBOLS + k) for k, n in enumerate(_fib(RARE_SYMBOLS + 1)[1:])])
    a = rng.permutation(a).tolist()
    seen = set()
    for i in range(2, len(a)):                               # a word that was there before: take a later byte in its place
        j = i
        while (a[i - 2], a[i - 1], a[j]) in seen:
            j += 1
        a[i], a[j] = a[j], a[i]
        seen.add((a[i - 2], a[i - 1], a[i]))
    return bytes(a)


def huffman_depth(hist):
    """the longest code of an unlimited Huffman code over the counts of `hist` (a dict symbol -> count)"""
    import heapq
    heap = [(n, 0) for n in hist.values() if n]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, da), (b, db) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def _de_bruijn(k, n):
    """every word of n letters over k letters once, no word twice: nothing to match, few symbols — a dynamic block without distance code"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return bytes(97 + x for x in seq + seq[:n - 1])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes; none is larger than one block but the record streams and 'three_blocks_and_one'"""
    rng = np.random.RandomState(1951)
    c = OrderedDict()
    for n in (0, 1, 2, 3, 4):
        c['len_%d' % n] = rng.randint(0, 256, n).astype(np.uint8).tobytes()
    for n in (258, 259, 260):
        c['equal_%d' % n] = b'\x07' * n
    c['zeros_65280'] = b'\x00' * BLOCK
    c['bytes_256_shuffled'] = rng.permutation(256).astype(np.uint8).tobytes()
    c['random_65280'] = rng.randint(0, 256, BLOCK).astype(np.uint8).tobytes()
    for P in PERIODS:
        c['period_%d' % P] = _period(rng, P)
    for P in PERIODS:                                        # the same, cut so that the last match would run 1, 2 or 3 bytes past the end
        for cut in (1, 2, 3):
            c['period_%d_cut_%d' % (P, cut)] = _period(rng, P, BLOCK - 3 + cut)
    for P in (1, 3, TILE, 258):                              # ... and a short one: two matches of 258 behind the first tile, then the cut
        for cut in (1, 2, 3):
            c['period_%d_short_cut_%d' % (P, cut)] = _period(rng, P, P + TILE + 2 * 258 + cut)
    c['fibonacci_literals'] = _fibonacci()
    c['fibonacci_over_flat_literals'] = _fibonacci_over_flat()
    c['alphabet16'] = bref._alphabet16()
    c['de_bruijn_5_3'] = _de_bruijn(5, 3)
    for f in bref.FIXTURE_BAMS:
        c['bam_' + f[:-4]] = gzip.open(os.path.join(GOLD, f)).read()
    c['three_blocks_and_one'] = bref._alphabet16(3 * BLOCK + 1, 31)
    c['exactly_one_block'] = bref._alphabet16(BLOCK, 32)
    return c


def fuzz_cases(directory):
    """name -> the record stream of a _bam_fuzz BAM"""
    return OrderedDict(('fuzz_%d' % s, gzip.open(_bam_fuzz.make_case(s, directory).bam).read()) for s in FUZZ_SEEDS)


def program_input(name, data):
    """what the sanitized program's run with 64 lanes gets of a case: all of it, except of the long record stream"""
    return data[:LONG_HEAD] + data[-LONG_TAIL:] if name == LONG_CASE else data


# ------------------------------------------------------------------------------------------------ a Python reading of DEFLATE streams
class _Bits(object):
    def __init__(self, data):
        self.d, self.p = data, 0

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v

    def symbol(self, table):
        code, n = 0, 0
        while True:
            code = (code << 1) | self.take(1); n += 1
            s = table.get((code, n))
            if s is not None:
                return s
            assert n <= 15, 'no code'


def _table(lens):
    return {v: s for s, v in bref.canon_codes(lens).items()}


def walk(payload):
    """[dict(type 0/1/2, len_syms, dist_syms, ll_lens, d_lens, cl_lens (sets of the code lengths in use), n_dist_codes, spelled_runs,
    ll_hist, d_hist (symbol -> count; of a stored block empty))]
    per block of a raw DEFLATE stream; the stream must end in the last byte"""
    b, out = _Bits(payload), []
    while True:
        final, typ = b.take(1), b.take(2)
        blk = dict(type=typ, len_syms=set(), dist_syms=set(), ll_lens=set(), d_lens=set(), cl_lens=set(), n_dist_codes=None, spelled_runs=0,
                   ll_hist={}, d_hist={})
        out.append(blk)
        assert typ != 3
        if typ == 0:
            b.p = (b.p + 7) & ~7
            n, nn = b.take(16), b.take(16)
            assert n == nn ^ 0xffff
            b.p += 8 * n
        else:
            if typ == 1:
                ll, d = bref.FIXED_LL, bref.FIXED_D
                ll, d = {v: s for s, v in ll.items()}, {v: s for s, v in d.items()}
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl = [0] * 19
                for s in CL_ORDER[:hclen]:
                    cl[s] = b.take(3)
                blk['cl_lens'] = set(x for x in cl if x)
                clt, lens = _table(cl), []
                while len(lens) < hlit + hdist:
                    s = b.symbol(clt)
                    if s < 16:
                        lens.append(s)
                    else:
                        blk['spelled_runs'] += 1
                        lens += [lens[-1]] * (3 + b.take(2)) if s == 16 else [0] * ((3 + b.take(3)) if s == 17 else (11 + b.take(7)))
                assert len(lens) == hlit + hdist
                lll, dl = lens[:hlit], lens[hlit:]
                blk['ll_lens'], blk['d_lens'] = set(x for x in lll if x), set(x for x in dl if x)
                blk['n_dist_codes'] = sum(1 for x in dl if x)
                assert lll[256], 'no end-of-block code'
                ll, d = _table(lll), _table(dl)
            while True:
                s = b.symbol(ll)
                blk['ll_hist'][s] = blk['ll_hist'].get(s, 0) + 1
                if s == 256:
                    break
                if s > 256:
                    assert s <= 285
                    blk['len_syms'].add(s)
                    b.take(LEN_EXTRA[s - 257])
                    ds = b.symbol(d)
                    assert ds <= 29
                    blk['dist_syms'].add(ds)
                    blk['d_hist'][ds] = blk['d_hist'].get(ds, 0) + 1
                    b.take(DIST_EXTRA[ds])
        if final:
            break
    assert (b.p + 7) >> 3 == len(payload), 'bytes behind the stream'
    return out


def fixed_literal_cost(data):
    """bytes of one fixed-Huffman block per 0xff00 input bytes that codes every byte as a literal, with the BGZF frame: what a compressor
    that finds no match and builds no code would write"""
    total = 0
    for k in range(0, len(data), BLOCK):
        part = np.frombuffer(data[k:k + BLOCK], np.uint8)
        bits = 3 + 7 + 8 * int((part < 144).sum()) + 9 * int((part >= 144).sum())
        total += (bits + 7) // 8 + 26
    return total


# ------------------------------------------------------------------------------------------ the deflate body on the host, sanitized
def build_host_program(directory, sanitize=True):
    """tests/c_host/bgzf_deflate_check.cc as an ordinary host program (its own main), with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(directory, 'bgzf_deflate_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-pthread', '-Wno-unknown-pragmas', '-I' + CSRC, os.path.join(ROOT, 'tests', 'c_host', 'bgzf_deflate_check.cc'),
           '-o', exe]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    subprocess.run(cmd, check=True)
    return exe


_ENV = dict(ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')


def host_run(exe, data, directory, tag='case', mode='blocks'):
    """-> (BGZF bytes of the blocks, [(len, stream length, form)] per block) of one run; a sanitizer report or a failed check fails it.
    mode 'blocks': one lane and 64 lanes; 'blocks1': one lane only"""
    src, dst = os.path.join(directory, tag + '.raw'), os.path.join(directory, tag + '.bgzf')
    with open(src, 'wb') as fh:
        fh.write(data)
    p = subprocess.run([exe, mode, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **_ENV))
    assert p.returncode == 0 and not p.stderr, 'bgzf_deflate_check failed (%d):\n%s' % (p.returncode, p.stderr.decode()[-4000:])
    rows = [tuple(int(x) for x in l.split()[1:]) for l in p.stdout.decode().splitlines()]
    return open(dst, 'rb').read(), rows


def lengths_run(exe):
    """the code-length builder's own mode: the lines it prints; a failed check fails it"""
    p = subprocess.run([exe, 'lengths'], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **_ENV))
    assert p.returncode == 0 and not p.stderr, 'bgzf_deflate_check lengths failed (%d):\n%s\n%s' % (p.returncode, p.stdout.decode(), p.stderr.decode()[-4000:])
    return p.stdout.decode().splitlines()
