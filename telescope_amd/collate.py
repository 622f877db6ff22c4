"""`--collate host | device` of the device loader: a BAM whose records are not name-collated (coordinate-sorted, as aligners and
pipelines hand it out) is brought into the order the loader reads, every alignment of a query name in one run of records.

The contract (include/telescope_em.h, tsem_bam_collate): the groups of records with equal names stand in the order of their first
records, and inside a group the records keep their input order; every record is the same bytes.  A file that is collated already
comes back unchanged.

The step is not streamed: the whole inflated record stream is read into host memory, and with `device` it is held twice in device
memory as well (input and output) beside 44 to 60 B per record, for the time of the step.  A file that does not fit is an error that
says so; collate such a file beforehand.
"""
import logging as lg
from time import perf_counter

import numpy as np

from ._lib import bam_collate, bam_scan

LAST = {}


class _Stream(object):
    """the `read(n)` that loader_device.bam_chunks asks of its file handle, over a uint8 array"""

    def __init__(self, data, inner):
        self._mv, self._p, self._inner = memoryview(data), 0, inner

    def read(self, n=-1):
        end = len(self._mv) if n is None or n < 0 else min(len(self._mv), self._p + n)
        out = bytes(self._mv[self._p:end])
        self._p = end
        return out

    def close(self):
        self._inner.close()

    def __getattr__(self, name):                             # (fallbacks, blocks, times() of bgzf.DeviceBgzfReader)
        return getattr(self._inner, name)


def collated_stream(fh, path, how, device=0, hash_bits=0):
    """`fh`: an inflated BAM stream behind its header (gzip's reader or bgzf.DeviceBgzfReader).  Reads the rest of it, collates the
    records on the host (how='host', one core) or on GPU `device` (how='device') and returns an object with the `read(n)` that
    bam_chunks uses; closing it closes `fh`.  LAST holds records, names, moved, seconds and (device) ms of the step.  The whole
    inflated stream is held in host memory, and for how='device' twice in device memory, during the step."""
    global LAST
    if how not in ('host', 'device'):
        raise ValueError("collate must be 'none', 'host' or 'device', not %r" % (how,))
    t0 = perf_counter()
    pieces = []
    while True:
        b = fh.read(64 << 20)
        if not b:
            break
        pieces.append(b)
    data = pieces[0] if len(pieces) == 1 else b''.join(pieces)
    del pieces
    t1 = perf_counter()
    off, used = bam_scan(data)
    if used != len(data):
        raise ValueError(('%s: truncated BAM record' if len(data) - used < 4 else '%s: truncated BAM') % path)
    try:
        out, order, names, ms = bam_collate(data, off, device=device if how == 'device' else None, hash_bits=hash_bits)
    except ValueError as e:
        raise ValueError('%s: %s' % (path, e))
    n = len(order)
    moved = int(np.count_nonzero(order != np.arange(n)))
    t2 = perf_counter()
    LAST = dict(how=how, records=n, names=names, moved=moved, read_s=t1 - t0, collate_s=t2 - t1, ms=ms)
    lg.info('collate (%s): %d records, %d names, %d records moved, %.2f s' % (how, n, names, moved, t2 - t1))
    return _Stream(out, fh)
