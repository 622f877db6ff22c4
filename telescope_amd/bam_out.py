"""BAM output of `--updated_sam` (model.py:214-285 `_load_sequential`, :479-521 `update_sam`), stdlib only.

  * `BgzfWriter`: BGZF blocks (zlib raw deflate, at most 64 KiB each) and the EOF block;
  * `BamWriter`: the BAM header (text + the input's binary reference list) and raw records, or pieces of an already framed record
    stream (`write_framed`: what the device rewrite of `--rewrite device` hands over);
  * `set_tag` / `get_tag` / `set_flag` / `set_mapq`: edits of a record's raw bytes (as `read_bam(..., raw=True)` yields them)
    that change the flag, the MAPQ and the tags and re-encode nothing else.  `set_tag` is pysam's `AlignedSegment.set_tag`:
    an existing tag of that name is deleted and the new one APPENDED; a Python int gets the smallest type that holds it
    (C, S, I for >= 0; c, s, i below), a str type Z;
  * `phred_table()`: where the reference's PHRED score steps.  helpers.py:14-37 computes it as numpy's scalar expression
    `int(round(-10 * np.log10(1 - P)))` (255 at P >= 1); numpy may pick its log10 kernel by CPU, so no device log10 can promise
    the same integers.  The table holds, for q = 1 .. phred(prevfloat(1)), the smallest float64 P with phred(P) >= q, found with
    that very expression by bisection over the bit patterns of [0, 1) and checked at +-2 ulp of every step; phred(P) is then
    the number of entries <= P.  The device tag pass (tsem_entry_tags) and `phred_lookup` read it.
"""
import struct
import zlib

import numpy as np

BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
_BLOCK_IN = 0xff00                      # input bytes per block: the deflated block stays below 64 KiB even when stored
_INT_TYPES = (('C', 0, 0xff), ('S', 0, 0xffff), ('I', 0, 0xffffffff))
_SINT_TYPES = (('c', -0x80, 0x7f), ('s', -0x8000, 0x7fff), ('i', -0x80000000, 0x7fffffff))
_FMT = {'c': '<b', 'C': '<B', 's': '<h', 'S': '<H', 'i': '<i', 'I': '<I', 'f': '<f'}
_B_SIZE = {'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4, 'f': 4}

FSECONDARY = 0x100
# colors.py: c2str of GPAL[2] (greens), D2PAL yellow / vermilion, and the grey of a SEC alignment (model.py:501-517)
YC_SEC, YC_ASSIGNED, YC_HIGH, YC_LOW = '248,248,248', '217,95,2', '230,171,2', '209,236,228'


# ------------------------------------------------------------------------------------------------------------- BGZF / BAM
class BgzfWriter(object):
    def __init__(self, path, level=6):
        self._fh = open(path, 'wb')
        self._buf = bytearray()
        self._level = level

    def write(self, data):
        """the stream is cut every _BLOCK_IN bytes however the bytes arrive; whole blocks of a large piece are deflated straight from
        it, without a pass through the buffer"""
        mv = memoryview(data).cast('B')
        p, n = 0, len(mv)
        if self._buf:
            p = min(n, _BLOCK_IN - len(self._buf))
            self._buf += mv[:p]
            if len(self._buf) < _BLOCK_IN:
                return
            self._block(bytes(self._buf))
            self._buf = bytearray()
        while n - p >= _BLOCK_IN:
            self._block(bytes(mv[p:p + _BLOCK_IN]))
            p += _BLOCK_IN
        self._buf += mv[p:]

    def _block(self, data):
        co = zlib.compressobj(self._level, zlib.DEFLATED, -15)
        comp = co.compress(data) + co.flush()
        if len(comp) + 25 >= 1 << 16:                       # incompressible: a stored block fits
            co = zlib.compressobj(0, zlib.DEFLATED, -15)
            comp = co.compress(data) + co.flush()
        self._fh.write(b'\x1f\x8b\x08\x04' + struct.pack('<IBBH', 0, 0, 0xff, 6) + b'BC' + struct.pack('<HH', 2, len(comp) + 25))
        self._fh.write(comp + struct.pack('<II', zlib.crc32(data) & 0xffffffff, len(data)))

    def close(self):
        if self._fh is None:
            return
        if self._buf:
            self._block(bytes(self._buf))
            self._buf = bytearray()
        self._fh.write(BGZF_EOF)
        self._fh.close()
        self._fh = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class BamWriter(object):
    """`header`: the dict `read_bam(..., raw=True)` returns (text, refs_block); records go in as raw bytes (no block size).
    `deflate`: 'host' (zlib level 6 on this core) or 'device' (`--deflate device`: the blocks are deflated on GPU `device`,
    bgzf.DeviceBgzfWriter; the same cuts and the same inflated bytes, other compressed ones)."""

    def __init__(self, path, header, text=None, deflate='host', device=0):
        if deflate not in ('host', 'device'):
            raise ValueError("deflate must be 'host' or 'device', not %r" % (deflate,))
        if deflate == 'device':
            from . import bgzf                              # (only here: this module's default path needs the standard library alone)
            self._z = bgzf.DeviceBgzfWriter(path, device=device)
        else:
            self._z = BgzfWriter(path)
        self.deflate = deflate
        t = (header['text'] if text is None else text).encode()
        try:
            self._z.write(b'BAM\x01' + struct.pack('<i', len(t)) + t + header['refs_block'])
        except BaseException:
            self._z.close()
            raise

    def device_stats(self):
        """(blocks, batches, tsem_bgzf_deflate_times) of a 'device' writer so far, None for a 'host' one"""
        return (self._z.blocks, self._z.batches, self._z.times()) if self.deflate == 'device' else None

    def write(self, rec):
        self._z.write(struct.pack('<i', len(rec)) + rec)

    def write_framed(self, stream):
        """a piece of an already framed stream (records with their block_size, cut anywhere): bytes, a memoryview or a uint8 array"""
        self._z.write(stream)

    def close(self):
        self._z.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def sum_device_stats(writers):
    """dict(deflate_blocks, deflate_batches, deflate_ms) over BamWriters with deflate='device' (closed ones too)"""
    out = dict(deflate_blocks=0, deflate_batches=0, deflate_ms=dict(h2d=0., k_bgzf_deflate=0., pack=0., d2h=0.))
    for w in writers:
        blocks, batches, ms = w.device_stats()
        out['deflate_blocks'] += blocks
        out['deflate_batches'] += batches
        for k in out['deflate_ms']:
            out['deflate_ms'][k] += ms[k]
    return out


def header_with_pg(text, version, command_line):
    """The input's header text plus ONE `@PG` line (ID telescope, or telescope.1, .2, ... where the header already holds that ID)."""
    ids = set()
    for line in text.splitlines():
        if line.startswith('@PG'):
            for f in line.split('\t')[1:]:
                if f.startswith('ID:'):
                    ids.add(f[3:])
    pid, i = 'telescope', 0
    while pid in ids:
        i += 1
        pid = 'telescope.%d' % i
    if text and not text.endswith('\n'):
        text += '\n'
    return text + '@PG\tID:%s\tPN:telescope\tVN:%s\tCL:%s\n' % (pid, version, command_line)


# -------------------------------------------------------------------------------------------------- raw record edits
def _aux_start(rec):
    l_rn, n_cig, l_seq = rec[8], struct.unpack_from('<H', rec, 12)[0], struct.unpack_from('<i', rec, 16)[0]
    return 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq


def _tag_end(rec, p):
    """end of the tag that starts at p"""
    typ = chr(rec[p + 2])
    q = p + 3
    if typ in _B_SIZE:
        return q + _B_SIZE[typ]
    if typ == 'A':
        return q + 1
    if typ in 'ZH':
        return rec.index(b'\x00', q) + 1
    if typ == 'B':
        (cnt,) = struct.unpack_from('<i', rec, q + 1)
        return q + 5 + cnt * _B_SIZE[chr(rec[q])]
    raise ValueError('unknown BAM tag type %r' % typ)


def iter_tags(rec):
    """(name, type, start, end) of every tag of a raw record, in order"""
    p, n = _aux_start(rec), len(rec)
    while p < n:
        e = _tag_end(rec, p)
        yield rec[p:p + 2].decode(), chr(rec[p + 2]), p, e
        p = e


def get_tag(rec, name):
    """value of a Z / integer / float tag (None where the record has no such tag)"""
    for t, typ, s, e in iter_tags(rec):
        if t == name:
            if typ in 'ZH':
                return rec[s + 3:e - 1].decode()
            if typ == 'A':
                return chr(rec[s + 3])
            if typ in _FMT:
                return struct.unpack_from(_FMT[typ], rec, s + 3)[0]
            return rec[s + 3:e]
    return None


def encode_tag(name, value):
    if isinstance(value, str):
        return name.encode() + b'Z' + value.encode() + b'\x00'
    if isinstance(value, (int, np.integer)) and not isinstance(value, bool):
        v = int(value)
        for typ, lo, hi in (_INT_TYPES if v >= 0 else _SINT_TYPES):
            if lo <= v <= hi:
                return name.encode() + typ.encode() + struct.pack(_FMT[typ], v)
        raise ValueError('integer tag %s=%d does not fit 32 bits' % (name, v))
    if isinstance(value, float):
        return name.encode() + b'f' + struct.pack('<f', value)
    raise TypeError('tag %s: unsupported value %r' % (name, value))


def set_tag(rec, name, value):
    """pysam's set_tag(name, value): the old tag (if any) goes, the new one is appended -> new record bytes"""
    a = _aux_start(rec)
    out = bytearray(rec[:a])
    for t, _typ, s, e in iter_tags(rec):
        if t != name:
            out += rec[s:e]
    out += encode_tag(name, value)
    return bytes(out)


def flag_of(rec):
    return struct.unpack_from('<H', rec, 14)[0]


def set_flag(rec, flag):
    return rec[:14] + struct.pack('<H', flag) + rec[16:]


def set_mapq(rec, mapq):
    return rec[:9] + bytes((mapq,)) + rec[10:]


def qname_of(rec):
    return rec[32:32 + rec[8] - 1].decode()


def record_text(rec):
    """canonical text of a record for comparisons: qname, flag, MAPQ, then every tag as NAME:TYPE:VALUE in order"""
    out = [qname_of(rec), str(flag_of(rec)), str(rec[9])]
    for t, typ, s, e in iter_tags(rec):
        if typ in 'ZH':
            v = rec[s + 3:e - 1].decode()
        elif typ == 'A':
            v = chr(rec[s + 3])
        elif typ in _FMT:
            v = repr(struct.unpack_from(_FMT[typ], rec, s + 3)[0])
        else:
            sub = chr(rec[s + 3])
            (cnt,) = struct.unpack_from('<i', rec, s + 4)
            v = sub + ',' + ','.join(str(x) for x in struct.unpack_from('<%d%s' % (cnt, _FMT[sub][1]), rec, s + 8))
        out.append('%s:%s:%s' % (t, typ, v))
    return '\t'.join(out)


# --------------------------------------------------------------------------------------------------------- PHRED
def phred_scalar(P):
    """helpers.py:14-37, verbatim"""
    return int(round(-10 * np.log10(1 - P))) if P < 1.0 else 255


def _f(bits):
    return float(np.uint64(bits).view(np.float64))


_PHRED_TAB = None


def phred_table():
    """float64[n]: tab[q - 1] = the smallest P in [0, 1) with phred_scalar(P) >= q (see the module docstring; q values the
    expression skips near P = 1 give equal entries).  Raises
    RuntimeError if numpy's expression is not monotone around a step (the table would not reproduce it)."""
    global _PHRED_TAB
    if _PHRED_TAB is not None:
        return _PHRED_TAB
    one = int(np.float64(1.0).view(np.uint64))
    qmax = phred_scalar(_f(one - 1))
    tab = []
    lo = 0
    for q in range(1, qmax + 1):
        a, b = lo, one - 1                                  # phred(_f(b)) >= q; find the least such bit pattern
        while a < b:
            m = (a + b) // 2
            if phred_scalar(_f(m)) >= q:
                b = m
            else:
                a = m + 1
        tab.append(_f(a))
        lo = a
    tab = np.array(tab, dtype=np.float64)
    if len(tab) >= 256 or np.any(np.diff(tab) < 0):                # (near P = 1 a step can skip values of q: equal entries)
        raise RuntimeError('phred_table: %d steps, not ascending' % len(tab))
    bits = tab.view(np.uint64).astype(np.int64)
    for d in (-2, -1, 0, 1, 2):
        p = np.array([_f(min(max(int(b) + d, 0), one - 1)) for b in bits])
        got = phred_lookup(p, tab)
        want = np.array([phred_scalar(x) for x in p])
        if not np.array_equal(got, want):
            bad = int(np.flatnonzero(got != want)[0])
            raise RuntimeError('phred_table: the table gives %d, numpy %d at P = %r (step %d %+d ulp)'
                               % (got[bad], want[bad], p[bad], bad + 1, d))
    _PHRED_TAB = tab
    return tab


def phred_lookup(p, tab=None):
    """phred_scalar of every p from the table (host restatement of the device lookup)"""
    tab = phred_table() if tab is None else tab
    p = np.asarray(p, dtype=np.float64)
    return np.where(p >= 1.0, 255, np.searchsorted(tab, p, side='right')).astype(np.int64)


def tag_word(z, assigned, tab=None):
    """the tag word of tsem_entry_tags from z and the assignment value, on the host"""
    z = np.asarray(z, dtype=np.float64)
    xp = np.rint(z * 100.0).astype(np.uint32)
    return (phred_lookup(z, tab).astype(np.uint32) | (xp << 8) | ((np.asarray(assigned) > 0).astype(np.uint32) << 16)
            | ((z >= 0.2).astype(np.uint32) << 17))


def decode_word(w):
    """-> (mapq, XP, assigned, z >= 0.2)"""
    w = int(w)
    return w & 0xff, (w >> 8) & 0xff, bool(w >> 16 & 1), bool(w >> 17 & 1)


def update_pair(recs, zt, fidx_word):
    """update_sam (model.py:495-518) on the raw records of ONE mapped AlignedPair (r1[, r2]).  `zt`: its ZT tag; `fidx_word`: the
    tag word of its (row, ZF) entry (0 where the entry is not stored: z = 0, unassigned).  -> new records"""
    out = []
    if zt == 'SEC':
        for r in recs:
            r = set_flag(r, flag_of(r) | FSECONDARY)
            r = set_tag(r, 'YC', YC_SEC)
            out.append(set_mapq(r, 0))
        return out
    mapq, xp, assigned, high = decode_word(fidx_word)
    for r in recs:
        r = set_mapq(r, mapq)
        r = set_tag(r, 'XP', xp)
        if assigned:
            r = set_flag(r, flag_of(r) & ~FSECONDARY)
            r = set_tag(r, 'YC', YC_ASSIGNED)
        else:
            r = set_flag(r, flag_of(r) | FSECONDARY)
            r = set_tag(r, 'YC', YC_HIGH if high else YC_LOW)
        out.append(r)
    return out
