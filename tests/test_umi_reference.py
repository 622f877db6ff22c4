"""The host definition of the UMI collapse (tests/_umi_reference.py): hand cases with the expected representatives written out, and
the vectorised form against the plain one on the random cases of the GPU tests."""
import numpy as np
import pytest

from _umi_reference import dedup_plain, dedup_vectorised, ground, random_case


def _csr(rows):
    """rows: a list of [(column, code), ...]"""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.array([c for r in rows for c, _ in r], np.int32)
    data = np.array([v for r in rows for _, v in r], np.uint16)
    return indptr, indices, data


# name -> (rows, cell_of_row, umi_of_row, expected rep, expected stats)
HAND = {
    'chain A-B-C: A and C share no column': (
        [[(0, 5), (1, 5)], [(1, 4), (2, 4)], [(2, 9), (3, 1)]], [0, 0, 0], [0, 0, 0], [2, 2, 2], [3, 1, 1, 2]),
    'same UMI in two cells is not merged': (
        [[(0, 5)], [(0, 7)], [(0, 6)]], [0, 1, 0], [3, 3, 3], [2, 1, 2], [3, 2, 2, 1]),
    'same class, disjoint loci: not merged': (
        [[(0, 5), (1, 5)], [(2, 9), (3, 9)]], [0, 0], [0, 0], [0, 1], [2, 1, 2, 0]),
    'a score tie: the smallest row wins': (
        [[(4, 3)], [(4, 8), (5, 2)], [(5, 8)], [(4, 8)]], [2, 2, 2, 2], [1, 1, 1, 1], [1, 1, 1, 1], [4, 1, 1, 3]),
    'a higher score on a later row wins': (
        [[(0, 8)], [(0, 8)], [(0, 9)]], [0, 0, 0], [0, 0, 0], [2, 2, 2], [3, 1, 1, 2]),
    'cell -1 is in no class': (
        [[(0, 5)], [(0, 7)], [(0, 6)]], [-1, -1, 0], [0, 0, 0], [0, 1, 2], [1, 1, 1, 0]),
    'umi -1 is in no class': (
        [[(0, 5)], [(0, 7)], [(0, 6)]], [0, 0, 0], [-1, 1, 1], [0, 1, 1], [2, 1, 1, 1]),
    'an empty row is a component by itself': (
        [[(0, 5)], [], [(0, 7)], []], [0, 0, 0, 0], [0, 0, 0, 0], [2, 1, 2, 3], [4, 1, 3, 1]),
    'unsorted column ids': (
        [[(7, 1), (2, 6), (5, 1)], [(9, 3), (5, 2)], [(3, 9), (9, 1), (0, 1)]], [0, 0, 0], [4, 4, 4], [2, 2, 2], [3, 1, 1, 2]),
}


@pytest.mark.parametrize('form', [dedup_plain, dedup_vectorised])
@pytest.mark.parametrize('name', sorted(HAND))
def test_hand_cases(name, form):
    rows, cell, umi, rep, stats = HAND[name]
    got_rep, got_stats = form(*_csr(rows), np.array(cell, np.int32), np.array(umi, np.int32))
    assert got_rep.dtype == np.int32 and got_rep.tolist() == rep, name
    assert got_stats.dtype == np.int64 and got_stats.tolist() == stats, name


def test_no_rows():
    for form in (dedup_plain, dedup_vectorised):
        rep, stats = form(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16), np.zeros(0, np.int32), np.zeros(0, np.int32))
        assert rep.shape == (0,) and stats.tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_two_forms_agree_on_the_random_cases(seed):
    indptr, indices, data, cell, umi, k = random_case(seed)
    rep, stats = dedup_plain(indptr, indices, data, cell, umi)
    vrep, vstats = dedup_vectorised(indptr, indices, data, cell, umi, k)
    assert np.array_equal(rep, vrep) and np.array_equal(stats, vstats)
    assert np.all(rep[rep] == rep)                           # a representative represents itself
    dropped, big, split = ground(indptr, indices, data, cell, umi)
    assert dropped >= 500 and big >= 100 and split >= 200, (dropped, big, split)
