"""The 3-byte entry index of the fused fp64 layouts (telescope_amd/csrc/tsem_idx24.h) on the host: tsem_debug_idx24 packs four
`lrow << 16 | lcol` words into the 12 bytes of a quad with the shared inline and unpacks them again.  No GPU."""
import itertools

import numpy as np
import pytest

from telescope_amd import _lib

ROWS = (0, 1, 1023, 1024, 1151, 2047)
COLS = (0, 1, 4095, 4096, 7679, 7743, 8191)


def _roundtrip(rc):
    rc = np.ascontiguousarray(rc, np.uint32)
    out = np.zeros(12, np.uint8)
    back = np.zeros(4, np.uint32)
    assert _lib.lib().tsem_debug_idx24(_lib.ptr(rc), _lib.ptr(out), _lib.ptr(back)) == _lib.OK
    return out, back


def _bits_reference(rc):
    """The layout written out independently: entry k is the 24-bit number lrow << 13 | lcol at bits 24k .. 24k+23 of a 96-bit
    little-endian integer."""
    big = 0
    for k, w in enumerate(int(x) for x in rc):
        big |= (((w >> 16) << 13) | (w & 0xFFFF)) << (24 * k)
    return np.frombuffer(big.to_bytes(12, 'little'), np.uint8)


@pytest.mark.parametrize('others', [0, 1], ids=['others-zero', 'others-ones'])
def test_every_field_in_every_position(others):
    fill = ((2047 << 16) | 8191) if others else 0
    for row, col, pos in itertools.product(ROWS, COLS, range(4)):
        rc = np.full(4, fill, np.uint32)
        rc[pos] = (row << 16) | col
        out, back = _roundtrip(rc)
        assert np.array_equal(back, rc), (row, col, pos, others)
        assert np.array_equal(out, _bits_reference(rc)), (row, col, pos, others)


def test_words_as_the_kernel_reads_them():
    """Three little-endian dwords: w0 = e0 | e1 << 24, w1 = e1 >> 8 | e2 << 16, w2 = e2 >> 16 | e3 << 8; an all-ones first word
    (the kernel's idle mark) can only come from row slot 2047."""
    rng = np.random.RandomState(24)
    for _ in range(200):
        rows, cols = rng.randint(0, 1152, 4), rng.randint(0, 7744, 4)
        rc = ((rows << 16) | cols).astype(np.uint32)
        out, back = _roundtrip(rc)
        e = [int(r) << 13 | int(c) for r, c in zip(rows, cols)]
        w = out.view('<u4')
        assert int(w[0]) == (e[0] | e[1] << 24) & 0xFFFFFFFF
        assert int(w[1]) == (e[1] >> 8 | e[2] << 16) & 0xFFFFFFFF
        assert int(w[2]) == (e[2] >> 16 | e[3] << 8) & 0xFFFFFFFF
        assert int(w[0]) != 0xFFFFFFFF
        assert np.array_equal(back, rc)
    out, _ = _roundtrip(np.array([(2047 << 16) | 8191, 255, 0, 0], np.uint32))
    assert int(out.view('<u4')[0]) == 0xFFFFFFFF
