"""The cases of the BGZF inflate tests (telescope_amd/bgzf.py, csrc/tsem_bgzf.hip, csrc/tsem_bgzf_inflate.h).  zlib is the oracle: every
valid payload is made by zlib or, bit by bit, by hand, and its expected bytes are zlib.decompress(payload, -15); every corrupt block
is shown to make Python's gzip refuse the member (a zlib error, a CRC or length mismatch, a premature end), so that no case rests on
this project's own reading of RFC 1951.  `build_host_program` / `host_run`: the inflate body as a stand-alone host program under the
address and undefined-behaviour sanitizers (tests/c_host/bgzf_inflate_check.cc)."""
import functools
import gzip
import os
import struct
import subprocess
import zlib
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'telescope_amd', 'csrc')
GOLD = os.path.join(ROOT, 'tests', 'golden')
FIXTURE_BAMS = ('loader_mixed.bam', 'sc_mixed.bam', 'sc_umi.bam', 'updated_mixed.bam', 'bundled_alignment.bam')
EOF_PAYLOAD = b'\x03\x00'
ST_HOST = 255

# payload: raw DEFLATE; expected: the inflated bytes (None for a corrupt case); status: the code the block must get (0: valid);
# isize / crc: the trailer's values where they are not those of `expected`
Case = namedtuple('Case', 'name payload expected status isize crc')


# ------------------------------------------------------------------------------------------------------------- the BGZF writer
def bgzf_block(payload, isize, crc, extra_in_front=b''):
    """one BGZF block around a raw DEFLATE payload; `extra_in_front`: other subfields ahead of BC"""
    extra = extra_in_front + b'BC\x02\x00' + struct.pack('<H', len(payload) + len(extra_in_front) + 6 + 19)
    blk = b'\x1f\x8b\x08\x04' + b'\x00' * 4 + b'\x00\xff' + struct.pack('<H', len(extra)) + extra + payload + struct.pack('<II', crc, isize)
    assert len(blk) <= 65536 and len(blk) == struct.unpack('<H', extra[-2:])[0] + 1
    return blk


def case_block(c, extra_in_front=b''):
    data = c.expected if c.expected is not None else b''
    return bgzf_block(c.payload, len(data) if c.isize is None else c.isize, zlib.crc32(data) if c.crc is None else c.crc, extra_in_front)


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, finish=zlib.Z_FINISH):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return z.compress(data) + z.flush(finish)


def valid(name, payload):
    expected = zlib.decompress(payload, -15)                 # the oracle; raises if the payload is not a valid stream
    return Case(name, payload, expected, 0, None, None)


def corrupt(name, payload, status, expected=None, isize=None, crc=None):
    c = Case(name, payload, expected, status, isize, crc)
    try:                                                     # gzip itself must refuse the member
        gzip.decompress(case_block(c))
    except (zlib.error, gzip.BadGzipFile, EOFError):
        return c
    raise AssertionError('case %s: gzip accepts the member' % name)


# ------------------------------------------------------------------------------------------------------- hand-built DEFLATE streams
class BitWriter(object):
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, n):
        """n bits, the lowest first (everything but Huffman codes)"""
        self.acc |= (value & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """a Huffman code of n bits, its first bit first"""
        for k in range(n - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def canon_codes(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s, ls in enumerate(lens):
            if ls == l:
                codes[s] = (code, l)
                code += 1
        code <<= 1
    return codes


FIXED_LL = canon_codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_D = canon_codes([5] * 32)


def emit(w, tokens, ll, d):
    """tokens: int (a literal / 256), ('m', length, distance), ('ll', symbol, extra bits, value), ('d', symbol, extra bits, value)"""
    for t in tokens:
        if isinstance(t, int):
            w.code(*ll[t])
        elif t[0] == 'm':
            _m, length, dist = t
            ls = 28 if length == 258 else max(i for i in range(28) if LEN_BASE[i] <= length)
            w.code(*ll[257 + ls]); w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
            ds = max(i for i in range(30) if DIST_BASE[i] <= dist)
            w.code(*d[ds]); w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        else:
            w.code(*(ll if t[0] == 'll' else d)[t[1]]); w.bits(t[3], t[2])


def stored(w, data, final):
    w.bits(final, 1); w.bits(0, 2); w.align()
    w.raw(struct.pack('<HH', len(data), len(data) ^ 0xFFFF) + data)


def fixed_stream(tokens, final=1, w=None):
    w = w or BitWriter()
    w.bits(final, 1); w.bits(1, 2)
    emit(w, tokens, FIXED_LL, FIXED_D)
    return w.bytes()


CL_LENS = [4] * 13 + [5] * 6                                 # a complete code over the 19 code-length symbols


def dynamic_stream(ll_lens, d_lens, cl_syms, tokens, cl_lens=CL_LENS, hclen=19, spelled_out=True):
    """one final dynamic block; cl_syms: [(symbol 0..18, value of its extra bits)] that spell ll_lens + d_lens (`spelled_out`)"""
    w = BitWriter()
    w.bits(1, 1); w.bits(2, 2)
    w.bits(len(ll_lens) - 257, 5); w.bits(len(d_lens) - 1, 5); w.bits(hclen - 4, 4)
    for s in CL_ORDER[:hclen]:
        w.bits(cl_lens[s], 3)
    cl = canon_codes(cl_lens)
    spelled, prev = [], None
    for s, x in cl_syms:
        w.code(*cl[s])
        if s < 16:
            spelled.append(s)
        elif s == 16:
            w.bits(x, 2); spelled += [spelled[-1]] * (3 + x)
        elif s == 17:
            w.bits(x, 3); spelled += [0] * (3 + x)
        else:
            w.bits(x, 7); spelled += [0] * (11 + x)
    assert not spelled_out or spelled == list(ll_lens) + list(d_lens), 'the code-length symbols do not spell the lengths'
    emit(w, tokens, canon_codes(ll_lens), canon_codes(d_lens))
    return w.bytes()


def _ab_lengths(eob=2, extra=()):
    """literal/length lengths over 'a' (2 bits), 'b' (2), end-of-block (`eob`), length symbols 257 and 258 (3 each), plus `extra`"""
    ll = [0] * 259
    ll[97], ll[98], ll[256], ll[257], ll[258] = 2, 2, eob, 3, 3
    for s, l in extra:
        ll[s] = l
    return ll


def _spell(lens):
    """the plainest spelling of a list of lengths: runs of zeros by 18 / 17, everything else literally"""
    out, i = [], 0
    while i < len(lens):
        if lens[i] == 0:
            j = i
            while j < len(lens) and lens[j] == 0 and j - i < 138:
                j += 1
            n = j - i
            out += [(18, n - 11)] if n >= 11 else [(17, n - 3)] if n >= 3 else [(0, 0)] * n
            i = j
        else:
            out.append((lens[i], 0)); i += 1
    return out


@functools.lru_cache(maxsize=None)
def hand_built_valid():
    rng = np.random.RandomState(285)
    cases = []
    # length symbol 285 and distance symbol 29 at distance 32,768, behind 32,768 stored bytes
    w = BitWriter()
    stored(w, rng.randint(0, 256, 32768).astype(np.uint8).tobytes(), 0)
    cases.append(valid('hand_fixed_285_dist_32768', fixed_stream([('m', 258, 32768), 256], 1, w)))
    # code lengths spelled with 16, 17 and 18; the 16 runs from the literal/length lengths (258) into the distance lengths (0, 1)
    ll, d = _ab_lengths(), [3, 3, 2, 1]
    syms = [(18, 97 - 11), (2, 0), (2, 0), (18, 127), (17, 7), (17, 6), (2, 0), (3, 0), (16, 0), (2, 0), (1, 0)]
    toks = [97, 98, 97, ('m', 3, 1), ('m', 4, 2), 98, ('m', 3, 3), ('m', 4, 4), 256]
    cases.append(valid('hand_dynamic_16_17_18_crossing', dynamic_stream(ll, d, syms, toks)))
    # one distance code of length 1: an incomplete set that RFC 1951 and zlib accept
    cases.append(valid('hand_dynamic_single_distance_code', dynamic_stream(ll, [1], _spell(ll + [1]), [97, ('m', 3, 1), 98, ('m', 4, 1), 256])))
    return tuple(cases)


def _alphabet16(n=65280, seed=16):
    return np.random.RandomState(seed).randint(0, 16, n).astype(np.uint8).tobytes().translate(bytes(range(65, 81)) + bytes(240))


@functools.lru_cache(maxsize=None)
def zlib_made():
    """name -> Case; the DEFLATE block types that zlib 1.2.11 produced for each are in the issue of this feature"""
    rng = np.random.RandomState(1951)
    a16 = _alphabet16()
    rnd = rng.randint(0, 256, 65280).astype(np.uint8).tobytes()
    cases = [valid('empty', EOF_PAYLOAD), valid('one_byte', deflate(b'x')), valid('size_65280', deflate(a16)),
             valid('level0_stored', deflate(a16, 0)), valid('fixed', deflate(a16, 6, zlib.Z_FIXED)),
             valid('level1', deflate(a16, 1)), valid('level6', deflate(a16, 6)), valid('level9', deflate(a16, 9)),
             valid('huffman_only', deflate(a16, 6, zlib.Z_HUFFMAN_ONLY)),
             valid('rle_equal_bytes', deflate(b'\x07' * 65280, 6, zlib.Z_RLE)),
             valid('incompressible', deflate(rnd, 6)),
             valid('long_distances', deflate(rnd[:32000] * 2, 9))]
    geo = np.concatenate([np.full(65000 >> (i + 1), i, np.uint8) for i in range(16)])
    rng.shuffle(geo)
    cases.append(valid('long_codes', deflate(geo.tobytes(), 6, zlib.Z_HUFFMAN_ONLY)))
    text = a16[:9000]
    for name, flush in (('sync_flush', zlib.Z_SYNC_FLUSH), ('full_flush', zlib.Z_FULL_FLUSH)):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 9)
        cases.append(valid(name, z.compress(text[:4001]) + z.flush(flush) + z.compress(text[4001:]) + z.flush(zlib.Z_FINISH)))
    # a change of strategy between the flushes: every compressor ends on a flush (an empty stored block on a byte boundary), the
    # last one finishes; no match of one reaches into another's bytes, so the concatenation is one valid stream
    mixed = (deflate(text[:3000], 6, zlib.Z_FIXED, zlib.Z_SYNC_FLUSH) + deflate(text[3000:6000], 6, zlib.Z_DEFAULT_STRATEGY, zlib.Z_FULL_FLUSH)
             + deflate(rnd[:2000], 0, zlib.Z_DEFAULT_STRATEGY, zlib.Z_SYNC_FLUSH) + deflate(text[6000:], 9, zlib.Z_HUFFMAN_ONLY))
    cases.append(valid('strategy_change', mixed))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def corrupt_cases():
    """one case per status code (more where the code names several things); the hand-built ones claim an ISIZE of 16, so that the
    output's bound is not what stops them"""
    good = valid('good', deflate(_alphabet16(3000, 3), 6))
    ll = _ab_lengths()
    over = _ab_lengths(extra=((99, 1),))                      # 1/2 + 3/4 + 1/4: over-subscribed
    no_eob = [0] * 257
    no_eob[97] = no_eob[98] = 1
    w = BitWriter(); w.bits(1, 1); w.bits(3, 2)
    w2 = BitWriter(); w2.bits(1, 1); w2.bits(0, 2); w2.align(); w2.raw(struct.pack('<HH', 5, 5) + b'hello')
    n = len(good.expected)
    return (corrupt('st1_block_type_3', w.bytes(), 1),
            corrupt('st2_stored_len_nlen', w2.bytes(), 2),
            corrupt('st3_oversubscribed_literal_length', dynamic_stream(over, [1], _spell(over + [1]), [97, 256]), 3),
            corrupt('st3_incomplete_distance', dynamic_stream(ll, [2, 2], _spell(ll + [2, 2]), [97, 256]), 3),
            corrupt('st3_incomplete_code_length_code', dynamic_stream(ll, [1], [], [], cl_lens=[1] + [0] * 18, spelled_out=False), 3),
            corrupt('st4_no_end_of_block', dynamic_stream(no_eob, [1], _spell(no_eob + [1]), [97, 98]), 4),
            corrupt('st5_symbol_286', fixed_stream([97, ('ll', 286, 0, 0), 256]), 5, isize=16),
            corrupt('st5_distance_30', fixed_stream([97, 98, 97, ('ll', 257, 0, 0), ('d', 30, 0, 0), 256]), 5, isize=16),
            corrupt('st6_distance_too_far', fixed_stream([97, ('m', 3, 2), 256]), 6, isize=16),
            corrupt('st7_longer_than_isize', good.payload, 7, good.expected, isize=n - 1),
            corrupt('st8_input_exhausted', good.payload[:-9], 8, good.expected),
            corrupt('st9_shorter_than_isize', good.payload, 9, good.expected, isize=n + 1),
            corrupt('st10_crc', good.payload, 10, good.expected, crc=zlib.crc32(good.expected) ^ 1))


def all_valid():
    return zlib_made() + hand_built_valid()


def oversize_case():
    """a gzip member with the BC subfield that claims more than 64 KiB inflated: the format forbids it, the host inflates it"""
    return valid('isize_100000', deflate(b'\x00' * 100000, 9))


@functools.lru_cache(maxsize=None)
def batch(n, seed=0):
    """(BGZF bytes, expected bytes, blocks) of n blocks of mixed sizes and levels, empty ones among them"""
    rng = np.random.RandomState(1000 + n + seed)
    sizes = [0, 1, 5, 100, 1000, 5000, 20000] if n > 65 else [0, 1, 17, 300, 4096, 30000, 65280]
    words = [bytes(rng.randint(65, 91, rng.randint(2, 12)).astype(np.uint8)) for _ in range(200)]
    blocks, exp = [], []
    for k in range(n):
        size = sizes[(k * 5 + rng.randint(0, 2)) % len(sizes)] if k else (sizes[-1] if n == 1 else 0)
        text = b' '.join(words[i] for i in rng.randint(0, 200, size // 4 + 1))[:size]
        c = valid('b%d' % k, EOF_PAYLOAD if size == 0 and k % 2 else deflate(text, (1, 6, 9, 0)[k % 4]))
        blocks.append(case_block(c)); exp.append(c.expected)
    return b''.join(blocks), b''.join(exp), tuple(blocks)


def corrupt_batch(c):
    """a corrupt block in the middle of valid ones: (BGZF bytes, [Case per block], its index)"""
    v = zlib_made()
    cs = [v[5], v[0], c, v[1], hand_built_valid()[1]]
    return b''.join(case_block(x) for x in cs), cs, 2


# --------------------------------------------------------------------------------------------------- a Python walk of the headers
def walk_headers(data):
    """(rows [block offset, payload offset, payload length, ISIZE, CRC-32], consumed, not_bgzf): what tsem_bgzf_scan must give"""
    rows, p = [], 0
    while p + 12 <= len(data):
        magic, xlen = data[p:p + 4], struct.unpack_from('<H', data, p + 10)[0]
        bsize = None
        if magic == b'\x1f\x8b\x08\x04':
            if p + 12 + xlen > len(data):
                break
            q, end = p + 12, p + 12 + xlen
            while q + 4 <= end:
                slen = struct.unpack_from('<H', data, q + 2)[0]
                if q + 4 + slen > end:
                    break
                if data[q:q + 2] == b'BC' and slen == 2:
                    bsize = struct.unpack_from('<H', data, q + 4)[0] + 1
                    break
                q += 4 + slen
        if bsize is None:
            if not rows:
                return [], 0, True
            raise ValueError('block %d at byte %d is no BGZF block' % (len(rows), p))
        if p + bsize > len(data):
            break
        crc, isize = struct.unpack_from('<II', data, p + bsize - 8)
        rows.append([p, p + 12 + xlen, bsize - xlen - 20, isize, crc])
        p += bsize
    return rows, p, False


# ------------------------------------------------------------------------------------------ the inflate body on the host, sanitized
def build_host_program(directory, sanitize=True):
    """tests/c_host/bgzf_inflate_check.cc as an ordinary host program (its own main), with the address and undefined-behaviour sanitizers"""
    exe = os.path.join(directory, 'bgzf_inflate_check')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-Wno-unknown-pragmas', '-I' + CSRC, os.path.join(ROOT, 'tests', 'c_host', 'bgzf_inflate_check.cc'),
           '-o', exe]
    if sanitize:
        cmd[1:1] = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-fno-omit-frame-pointer']
    subprocess.run(cmd, check=True)
    return exe


def host_run(exe, data, directory, tag='case'):
    """-> ((blocks, consumed, not_bgzf), [status per block], [output range per block]) of one run; a sanitizer report fails it"""
    src, dst = os.path.join(directory, tag + '.bgzf'), os.path.join(directory, tag + '.out')
    with open(src, 'wb') as fh:
        fh.write(data)
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=0', UBSAN_OPTIONS='print_stacktrace=1')
    p = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert p.returncode == 0 and not p.stderr, 'bgzf_inflate_check failed (%d):\n%s' % (p.returncode, p.stderr.decode()[-4000:])
    lines = p.stdout.decode().splitlines()
    assert lines and lines[0].startswith('scan '), lines[:1]
    scan = tuple(int(x) for x in lines[0].split()[1:])
    rows = [tuple(int(x) for x in l.split()) for l in lines[1:]]
    out = open(dst, 'rb').read()
    ranges, o = [], 0
    for _k, st, isize in rows:
        n = 0 if st == ST_HOST else isize
        ranges.append(out[o:o + n]); o += n
    assert o == len(out)
    return scan, [r[1] for r in rows], ranges
