"""BGZF inflate on the device (`assign --loader device --inflate device`; csrc/tsem_bgzf.hip, csrc/tsem_bgzf_inflate.h).

A BGZF file — every BAM file — is a chain of gzip members of at most 64 KiB that need nothing from each other.  The host walks the
chain of headers of a piece of the file (tsem_bgzf_scan), one device call inflates every whole block of the piece (k_bgzf_inflate: one
wave per block, CRC-32 and length checked against the trailer), and the partial block at the piece's end is carried into the next one.

  inflate(data)              a whole BGZF byte string -> bytes
  DeviceBgzfReader(path)     a readable binary file object over the inflated stream: what loader.read_bam_header and
                             loader_device.bam_chunks take in place of gzip.open(path)

The other direction (`assign --updated_sam --deflate device`; csrc/tsem_bgzf_deflate.h): a stream cut every 0xff00 bytes, every block
deflated by one wave (k_bgzf_deflate), header, stream and trailer of every block packed into one file image on the device.

  deflate(data)              bytes -> a whole BGZF byte string, EOF block included
  DeviceBgzfWriter(path)     a writable binary file object: what bam_out.BamWriter(deflate='device') writes through

A block whose trailer claims more than 65,536 inflated bytes (the format forbids it; a gzip member can say so) is inflated with zlib on
the host and counted in `fallbacks`.  A file that is gzip but not BGZF — no BC subfield in its first header, a BAM written by plain
gzip — is read with Python's gzip as the host path does, `inflate` of the reader says 'host'.
"""
import gzip
import io
import logging as lg
import zlib

import numpy as np

from ._lib import BGZF_BLOCK_IN, BGZF_HOST, BGZF_STATUS, BgzfDeflater, BgzfInflater, EngineError, bgzf_scan
from .bam_out import BGZF_EOF

DEFAULT_BATCH_BYTES = 64 << 20
MAX_BLOCK = 65536                      # bytes of a whole BGZF block at most: BSIZE is 16 bits


def _inflate_blocks(dev, piece, blocks, name, block0, offset0):
    """every block of `blocks` (rows of bgzf_scan over `piece`) -> (uint8 array of their bytes in order, blocks left to the host);
    block0 / offset0: the number and the file offset of the piece's first block, for the message"""
    out, st, (code, bad) = dev.inflate(piece, blocks)
    if code:
        raise ValueError('%s: BGZF block %d at byte %d: %s' % (name, block0 + bad, offset0 + int(blocks[bad, 0]),
                                                                BGZF_STATUS.get(code, 'status %d' % code)))
    hosted = np.flatnonzero(st == BGZF_HOST)
    if hosted.size == 0:
        return out, 0
    isz = np.where(st == BGZF_HOST, 0, blocks[:, 3])
    start = np.cumsum(isz) - isz                             # where each block's bytes begin in `out`
    parts, o = [], 0
    for k in hosted.tolist():
        po, pl, isize, crc = (int(x) for x in blocks[k, 1:5])
        try:
            raw = zlib.decompress(bytes(piece[po:po + pl]), -15)
        except zlib.error as e:
            raise ValueError('%s: BGZF block %d at byte %d: %s' % (name, block0 + k, offset0 + int(blocks[k, 0]), e))
        if len(raw) != isize or zlib.crc32(raw) != crc:
            raise ValueError('%s: BGZF block %d at byte %d: %s' % (name, block0 + k, offset0 + int(blocks[k, 0]),
                                                                    BGZF_STATUS[9 if len(raw) < isize else 7 if len(raw) > isize else 10]))
        parts += [out[o:int(start[k])], np.frombuffer(raw, np.uint8)]
        o = int(start[k])
    parts.append(out[o:])
    return np.concatenate(parts), int(hosted.size)


def inflate(data, device=0):
    """The inflated bytes of a whole BGZF byte string, every block on GPU `device` in one call.  ValueError: not BGZF, a truncated
    last block, a block that does not inflate (its number, its offset, why)."""
    data = bytes(data)
    try:
        blocks, used, not_bgzf = bgzf_scan(data)
    except EngineError as e:
        raise ValueError('<bytes>: %s' % e)
    if not_bgzf:
        raise ValueError('<bytes>: not BGZF (no 1f 8b 08 04 header with a BC subfield at the start)')
    if used != len(data):
        raise ValueError('<bytes>: truncated BGZF block')
    dev = BgzfInflater(device)
    try:
        out, _hosted = _inflate_blocks(dev, data, blocks, '<bytes>', 0, 0)
    finally:
        dev.close()
    return out.tobytes()


def deflate(data, device=0):
    """The whole BGZF byte string of `data`, EOF block included, every block deflated on GPU `device` in one call (the mirror of
    `inflate`): blocks of 0xff00 input bytes, the last one shorter, as bam_out.BgzfWriter cuts them."""
    dev = BgzfDeflater(device)
    try:
        out = dev.deflate(bytes(data))
    finally:
        dev.close()
    return out.tobytes() + BGZF_EOF


class DeviceBgzfWriter(object):
    """bam_out.BgzfWriter with the blocks deflated on the device (`--deflate device`; k_bgzf_deflate, one wave per block): write(data),
    close(), context manager.  The stream is cut every 0xff00 bytes however the bytes arrive, as BgzfWriter cuts it.  Whole blocks
    collect until `batch_bytes` of them are there (default 64 MiB) and go through one device call, which returns the finished file
    image of the batch; the partial block at the end goes at close(), followed by the EOF block.  `blocks`, `batches`: what went
    through the device so far; times(): tsem_bgzf_deflate_times."""

    def __init__(self, path, device=0, batch_bytes=DEFAULT_BATCH_BYTES):
        if int(batch_bytes) < 1:
            raise ValueError('batch_bytes must be >= 1')
        self.name, self.blocks, self.batches = path, 0, 0
        self._batch = max(1, int(batch_bytes) // BGZF_BLOCK_IN) * BGZF_BLOCK_IN     # whole blocks per device call
        self._buf, self._times = bytearray(), None
        self._dev = None
        self._fh = open(path, 'wb')
        try:
            self._dev = BgzfDeflater(device)
        except BaseException:
            self._release()
            raise

    def _release(self):
        if self._dev is not None:
            self._times = self._dev.times()
        for x in ('_fh', '_dev'):
            if getattr(self, x, None) is not None:
                getattr(self, x).close()
                setattr(self, x, None)

    def _send(self, n):
        """the first n bytes of the buffer through the device and into the file"""
        out = self._dev.deflate(memoryview(self._buf)[:n])
        self._fh.write(memoryview(out))
        self.blocks += (n + BGZF_BLOCK_IN - 1) // BGZF_BLOCK_IN
        self.batches += 1
        del out
        self._buf = self._buf[n:]

    def write(self, data):
        if self._fh is None:
            raise ValueError('write to a closed file')
        try:
            self._buf += memoryview(data).cast('B')
            while len(self._buf) >= self._batch:
                self._send(self._batch)
        except BaseException:
            self._release()
            raise

    def times(self):
        """dict(h2d, k_bgzf_deflate, pack, d2h in HIP-event milliseconds over the batches so far, batches)"""
        return self._dev.times() if self._dev is not None else dict(self._times or dict(h2d=0., k_bgzf_deflate=0., pack=0., d2h=0., batches=0))

    def close(self):
        if self._fh is None:
            return
        try:
            if self._buf:
                self._send(len(self._buf))
            self._fh.write(BGZF_EOF)
        finally:
            self._release()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class DeviceBgzfReader(object):
    """The inflated stream of the BGZF file `path` as a readable binary file object: read(n), close(), context manager.

    The file is read in pieces of `batch_bytes` compressed bytes (default 64 MiB); every whole block of a piece is inflated in one
    device call, the partial block at its end waits for the next piece.  A piece that holds no whole block grows to the 64 KiB a block
    can have at most before it is looked at again.  `inflate`: 'device', or 'host' for a gzip file that is not BGZF; `fallbacks`: blocks
    inflated by zlib on the host; `blocks`, `batches`: what went through the device so far; times(): tsem_bgzf_times."""

    def __init__(self, path, device=0, batch_bytes=DEFAULT_BATCH_BYTES):
        if int(batch_bytes) < 1:
            raise ValueError('batch_bytes must be >= 1')
        self.name, self.batch_bytes = path, int(batch_bytes)
        self.inflate, self.fallbacks, self.blocks, self.batches = 'device', 0, 0, 0
        self._dev = self._host = None
        self._cur, self._pos = np.zeros(0, np.uint8), 0
        self._tail, self._offset, self._eof, self._grow = b'', 0, False, False
        self._fh = open(path, 'rb')
        try:
            head = self._fh.read(MAX_BLOCK)                  # (a first header is whole within a block's 64 KiB)
            self._fh.seek(0)
            if bgzf_scan(head, cap=1)[2]:                    # gzip without the BC subfield, or no gzip at all: Python's gzip decides
                self._fh.close()
                self._fh = None
                self.inflate = 'host'
                lg.info('%s is not BGZF (no BC subfield in its first header): inflating on the host' % path)
                self._host = io.BufferedReader(gzip.open(path, 'rb'), buffer_size=1 << 20)
            else:
                self._dev = BgzfInflater(device)
        except BaseException:
            self.close()
            raise

    def _fill(self):
        """the next batch of inflated bytes into self._cur; False at the end of the file"""
        while True:
            if self._eof:
                return False
            new = self._fh.read(max(self.batch_bytes, MAX_BLOCK - len(self._tail)) if self._grow else self.batch_bytes)
            self._eof = not new
            data = self._tail + new if new else self._tail
            if self._eof and not data:
                return False
            try:
                blocks, used, not_bgzf = bgzf_scan(data)
            except EngineError as e:
                raise ValueError('%s: at byte %d: %s' % (self.name, self._offset, e))
            if not_bgzf:
                raise ValueError('%s: at byte %d: no BGZF header' % (self.name, self._offset))
            if len(blocks) == 0:
                if self._eof:
                    raise ValueError('%s: truncated BGZF block' % self.name)
                self._tail, self._grow = data, True
                continue
            self._grow = False
            out, hosted = _inflate_blocks(self._dev, data, blocks, self.name, self.blocks, self._offset)
            self.fallbacks += hosted
            self.blocks += len(blocks)
            self.batches += 1
            self._offset += used
            self._tail = data[used:]
            if out.size:
                self._cur, self._pos = out, 0
                return True

    def read(self, n=-1):
        if self._host is not None:
            return self._host.read(n)
        if self._dev is None:
            raise ValueError('read of a closed file')
        parts, need = [], (-1 if n is None or n < 0 else int(n))
        while need:
            if self._pos >= self._cur.size and not self._fill():
                break
            take = self._cur.size - self._pos if need < 0 else min(need, self._cur.size - self._pos)
            parts.append(self._cur[self._pos:self._pos + take].tobytes())
            self._pos += take
            if need > 0:
                need -= take
        return parts[0] if len(parts) == 1 else b''.join(parts)

    def readable(self):
        return True

    def times(self):
        """dict(h2d, k_bgzf_inflate, d2h in HIP-event milliseconds over the batches so far, batches); zeros for the host path"""
        return self._dev.times() if self._dev is not None else dict(h2d=0., k_bgzf_inflate=0., d2h=0., batches=0)

    def close(self):
        for x in ('_fh', '_host', '_dev'):
            if getattr(self, x, None) is not None:
                getattr(self, x).close()
                setattr(self, x, None)
        self._cur = np.zeros(0, np.uint8)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
