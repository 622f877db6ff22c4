"""The 8-byte quad index of the fused layouts with fp64 entries (telescope_amd/csrc/tsem_quad64.h), on the host, no GPU: a numpy model
of the word — 13-bit column slots at bits 0, 13, 26 and 39, the row steps d1, d2, d3 at bits 52-54, the first entry's row slot at bits
55-63 — against tsem_debug_quad64, which packs and unpacks with the inline functions the pack kernel and the fused kernel use."""
import ctypes as C
import itertools

import numpy as np
import pytest

from telescope_amd import _lib

COLS = (0, 4095, 4096, 7679)
ROW0 = (0, 255, 256, 508)
STEPS = tuple(itertools.product((0, 1), repeat=3))          # all eight step patterns


def _model_pack(rows, cols):
    w = 0
    for k in range(4):
        w |= int(cols[k]) << (13 * k)
    for k in range(1, 4):
        w |= int(rows[k] - rows[k - 1]) << (51 + k)
    return w | int(rows[0]) << 55


def _model_unpack(w):
    cols = [(w >> (13 * k)) & 0x1FFF for k in range(4)]
    rows = [w >> 55]
    for k in range(1, 4):
        rows.append(rows[-1] + ((w >> (51 + k)) & 1))
    return rows, cols


def _lib_quad(rows, cols, probe=0):
    """(return code, word, the four words unpacked again, whether `probe` names a stored quad)"""
    rc4 = np.array([(int(r) << 16) | int(c) for r, c in zip(rows, cols)], np.uint32)
    word, back = np.zeros(1, np.uint64), np.zeros(4, np.uint32)
    stored = C.c_int32(-1)
    rc = _lib.lib().tsem_debug_quad64(_lib.ptr(rc4), _lib.ptr(word), _lib.ptr(back), C.c_uint64(int(probe)), C.byref(stored))
    return rc, int(word[0]), back, stored.value, rc4


def test_symbol_is_declared_and_exported():
    assert 'tsem_debug_quad64' in _lib.exported_symbols()
    assert hasattr(_lib.lib(), 'tsem_debug_quad64')


@pytest.mark.parametrize('r0', ROW0)
def test_word_against_the_model(r0):
    """every step pattern x every rotation of the boundary columns, at the first row slots 0, 255, 256 and 508 (r3 reaches 511)"""
    seen_r3 = set()
    for steps in STEPS:
        rows = [r0, r0 + steps[0], r0 + steps[0] + steps[1], r0 + sum(steps)]
        seen_r3.add(rows[3])
        for shift in range(4):
            cols = [COLS[(k + shift) % 4] for k in range(4)]
            rc, word, back, _, rc4 = _lib_quad(rows, cols)
            assert rc == _lib.OK, (rows, cols)
            assert word == _model_pack(rows, cols), (rows, cols, hex(word))
            assert _model_unpack(word) == (rows, cols)
            assert np.array_equal(back, rc4), (rows, cols, back)        # the round trip to lrow << 16 | lcol
            # the fields, bit by bit
            assert (word >> 52) & 7 == steps[0] | steps[1] << 1 | steps[2] << 2 and word >> 55 == r0
    if r0 == 508:
        assert 511 in seen_r3


def test_every_column_bit_and_every_row_bit():
    for bit in range(13):
        c = 1 << bit
        for k in range(4):
            cols = [0, 0, 0, 0]
            cols[k] = c
            rc, word, back, _, rc4 = _lib_quad([5, 5, 6, 6], cols)
            assert rc == _lib.OK and word == _model_pack([5, 5, 6, 6], cols) and np.array_equal(back, rc4)
    for bit in range(9):
        r = 1 << bit
        rc, word, back, _, rc4 = _lib_quad([r, r, r, r + 1], [1, 2, 3, 4])
        assert rc == _lib.OK and word >> 55 == r and np.array_equal(back, rc4)


@pytest.mark.parametrize('rows', [(3, 5, 5, 5), (3, 3, 5, 5), (3, 4, 4, 6), (4, 3, 3, 3), (0, 0, 1, 0), (512, 512, 512, 512)])
def test_a_quad_the_format_cannot_hold_is_refused(rows):
    """a step of 2, a step down, a first row slot beyond 9 bits"""
    rc, _, _, _, _ = _lib_quad(rows, (1, 2, 3, 4))
    assert rc == _lib.ERR_ARG


def test_columns_beyond_the_field_are_refused():
    for k in range(4):
        cols = [0, 0, 0, 0]
        cols[k] = 8191                                          # the value the idle mark is made of
        assert _lib_quad((1, 1, 1, 1), cols)[0] == _lib.ERR_ARG
        cols[k] = 8192
        assert _lib_quad((1, 1, 1, 1), cols)[0] == _lib.ERR_ARG


def test_the_idle_mark_names_no_stored_quad():
    """a low half of 0xFFFFFFFF is the fused kernel's idle mark: it would need column slot 8191 twice, which no layout has"""
    for hi in (0, 1, 0x12345678, 0xFFFFFFFF):
        assert _lib_quad((0, 0, 0, 0), (0, 0, 0, 0), probe=(hi << 32) | 0xFFFFFFFF)[3] == 0
    rows, cols = _model_unpack(0xFFFFFFFF)
    assert cols[0] == 8191 and cols[1] == 8191
    # every word the packer produces is a stored quad, the largest columns and rows included
    for rows, cols in (((511, 511, 511, 511), (7679,) * 4), ((0, 0, 0, 0), (0,) * 4), ((508, 509, 510, 511), (8190,) * 4)):
        rc, word, _, _, _ = _lib_quad(rows, cols)
        assert rc == _lib.OK
        assert _lib_quad(rows, cols, probe=word)[3] == 1
