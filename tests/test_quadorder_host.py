"""The conflict-aware order inside the quads of the fused layouts with fp64 entries (telescope_amd/csrc/tsem_quadorder.h), on the host:
a numpy model of the rule written from its description — windows of 16 quads, per slot a count of the classes (column slot & 15) placed
so far, of the permutations that keep every position's row the one with the smallest sum of counts, ties to the first in lexicographic
order — against tsem_quad_order_host, which runs the inline functions the set-up kernel runs.  No device."""
from itertools import permutations

import numpy as np
import pytest

from telescope_amd import _lib

PERMS = sorted(permutations(range(4)))                       # lexicographic: the identity first
assert PERMS[0] == (0, 1, 2, 3)


def model(words):
    """[n windows x 64] row << 16 | column words -> [n x 16 x 4] the entry placed at each position of each quad"""
    words = np.asarray(words, np.uint32).reshape(-1, 16, 4)
    out = np.zeros(words.shape, np.int64)
    for w, win in enumerate(words):
        h = np.zeros((4, 16), np.int64)
        for l, quad in enumerate(win):
            row, cls = (quad >> 16).tolist(), (quad & 15).tolist()
            best, pick = None, None
            for p in PERMS if len(set(row)) < 4 else PERMS[:1]:
                if any(row[p[j]] != row[j] for j in range(4)):
                    continue
                s = sum(h[j, cls[p[j]]] for j in range(4))
                if best is None or s < best:
                    best, pick = s, p
            for j in range(4):
                h[j, cls[pick[j]]] += 1
            out[w, l] = pick
    return out


def decode(codes):
    codes = np.asarray(codes, np.int64)
    return np.stack([(codes >> (2 * j)) & 3 for j in range(4)], axis=-1).reshape(-1, 16, 4)


def apply(words, perm):
    words = np.asarray(words, np.uint32).reshape(-1, 16, 4)
    return np.take_along_axis(words, perm, axis=2)


def worst_multiplicity(words):
    """mean over (window, slot) of the largest number of the 16 lanes whose classes agree"""
    cls = (np.asarray(words, np.uint32).reshape(-1, 16, 4) & 15).astype(np.int64)
    n = cls.shape[0]
    cnt = np.zeros((n, 4, 16), np.int64)
    np.add.at(cnt, (np.repeat(np.arange(n), 64), np.tile(np.arange(4), 16 * n), cls.ravel()), 1)
    return float(cnt.max(axis=2).mean())


def rows_of_lengths(lens, rng, n_cols=7680, pad_to=64):
    """row-ordered words: row slots ascend with the rows, random column slots; padded to whole windows with the last row and column 0"""
    lens = np.asarray(lens, np.int64)
    row = np.repeat(np.arange(len(lens), dtype=np.int64) % 2048, lens)
    col = rng.randint(0, n_cols, row.size)
    pad = -row.size % pad_to
    row = np.concatenate([row, np.repeat(row[-1:], pad)])
    col = np.concatenate([col, np.zeros(pad, np.int64)])
    return ((row << 16) | col).astype(np.uint32)


def check(words, label):
    words = np.asarray(words, np.uint32)
    codes, moved = _lib.quad_order_host(words)
    got, want = decode(codes), model(words)
    w3 = words.reshape(-1, 16, 4)
    assert np.array_equal(np.sort(got, axis=2), np.broadcast_to(np.arange(4), got.shape)), (label, 'a permutation within the quad')
    out = apply(words, got)
    assert np.array_equal(out >> 16, w3 >> 16), (label, 'a position changed its row')
    distinct = np.array([[len(set(q.tolist())) == 4 for q in win] for win in (w3 >> 16)])
    assert np.all(got[distinct] == np.arange(4)), (label, 'four different rows: the identity')
    assert np.array_equal(got, want), (label, 'the library against the model', int((got != want).any(axis=2).sum()))
    assert moved == int((got != np.arange(4)).any(axis=2).sum()), label
    return out.reshape(-1), moved


@pytest.mark.parametrize('length', [1, 2, 3, 4, 5, 10, 70])
def test_rows_of_one_length(length):
    rng = np.random.RandomState(100 + length)
    words = rows_of_lengths(np.full(6400 // length + 1, length), rng)
    _, moved = check(words, 'length %d' % length)
    assert (moved > 0) == (length > 1), (length, moved)


def test_padding_and_equal_classes():
    rng = np.random.RandomState(5)
    # windows of nothing but padding: one row, column slot 0
    pad = np.full(4 * 64, 7 << 16, np.uint32)
    out, moved = check(pad, 'padding')
    assert moved == 0 and np.array_equal(out, pad)
    # every class equal, columns different: every permutation costs the same, the identity is first
    same = rows_of_lengths(np.full(64, 10), rng)
    same = (same & np.uint32(0xFFFF0000)) | ((same & np.uint32(0xFFFF)) // 16 * 16 + 3).astype(np.uint32)
    out, moved = check(same, 'one class')
    assert moved == 0 and np.array_equal(out, same)
    # rows that come back inside a quad (no layout has them; the rule reads equality of rows, not runs)
    mixed = rows_of_lengths(np.full(64, 10), rng).reshape(-1, 4)
    mixed[:, [1, 2]] = mixed[:, [2, 1]]
    check(mixed.reshape(-1), 'mixed')
    codes, moved = _lib.quad_order_host(np.zeros(0, np.uint32))
    assert codes.size == 0 and moved == 0
    with pytest.raises(ValueError):
        _lib.quad_order_host(np.zeros(63, np.uint32))


def test_effect_on_poisson_rows():
    """12 000 rows of Poisson(10) entries, uniform classes: the mean worst multiplicity per (window, slot) falls from >= 2.9 to <= 2.3
    (the model alone: 3.07 -> 2.15-2.18; 2.3 is what the walk over score-code rows reaches)"""
    rng = np.random.RandomState(2024)
    lens = np.maximum(1, rng.poisson(10, 12000))
    words = rows_of_lengths(lens, rng)
    codes, moved = _lib.quad_order_host(words)
    after = apply(words, decode(codes)).reshape(-1)
    assert np.array_equal(decode(codes)[:200], model(words[:200 * 64]))
    m0, m1 = worst_multiplicity(words), worst_multiplicity(after)
    print('QUADORDER poisson(10): %d windows, %d quads moved, worst multiplicity %.3f -> %.3f' % (words.size // 64, moved, m0, m1))
    assert m0 >= 2.9 and m1 <= 2.3, (m0, m1)


def test_symbol_and_info_names():
    assert 'tsem_quad_order_host' in _lib.exported_symbols() and hasattr(_lib.lib(), 'tsem_quad_order_host')
