"""The table of the fused kernel's instantiations (fz_exists, telescope_amd/csrc/tsem_fused.h), on the host, no GPU.  Every cell of
team size 1..8 x mode 0..9 x entry format 0..2 x geometry 0..3 x timeline x index format goes through tsem_debug_fused_cell: the
look-up the host launches through (fz_kernel, generated from the predicate) and the predicate itself must agree, and the cells that
exist must be the committed list.

tests/golden/fused_kernels.txt was recorded from the commit BEFORE the table became one predicate, through the same entry point
added to a scratch copy of it (its `quad` argument true for index format 2, false with index format fz_index(mode, fmt) otherwise).
That look-up answered 728 of the requests; 352 of them with the kernel of ANOTHER cell — mode 6 (which k_em_fused does not have) with
mode 2's, 64 requests; a geometry the team size does not have (0 or 3 for teams of 5-8, 1 for teams of 1-4) with a neighbouring
one's, 288 requests.  No call site could make such a request.  The list holds the other 376: one line per kernel, and exactly the
376 k_em_fused kernels of that commit's device code.  Requests for a cell that is not in the table now return no kernel."""
import ctypes as C
import itertools
import os

import pytest

from telescope_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fused_kernels.txt')
CELLS = tuple(itertools.product(range(1, 9), range(10), range(3), range(4), (0, 1), range(3)))


@pytest.fixture(scope='module')
def table():
    """cell -> (the look-up returns a kernel, the predicate lists it)"""
    L, out = _lib.lib(), {}
    for cell in CELLS:
        found, listed = C.c_int32(-1), C.c_int32(-1)
        assert L.tsem_debug_fused_cell(*cell, C.byref(found), C.byref(listed)) == _lib.OK
        assert found.value in (0, 1) and listed.value in (0, 1)
        out[cell] = (found.value, listed.value)
    return out


def test_symbol_is_declared_and_exported():
    assert 'tsem_debug_fused_cell' in _lib.exported_symbols()
    assert hasattr(_lib.lib(), 'tsem_debug_fused_cell')


def test_null_outputs_are_refused():
    found = C.c_int32(-1)
    assert _lib.lib().tsem_debug_fused_cell(1, 0, 0, 0, 0, 1, C.byref(found), None) == _lib.ERR_ARG
    assert _lib.lib().tsem_debug_fused_cell(1, 0, 0, 0, 0, 1, None, C.byref(found)) == _lib.ERR_ARG


def test_lookup_and_predicate_agree_on_every_cell(table):
    assert len(table) == 8 * 10 * 3 * 4 * 2 * 3
    assert [c for c, (found, listed) in table.items() if found != listed] == []


def test_existing_cells_are_the_committed_list(table):
    have = sorted('k_em_fused<%d, %d, %d, %d, %s, %d>' % (P, m, f, g, 'true' if t else 'false', x)
                  for (P, m, f, g, t, x), (found, _) in table.items() if found)
    want = open(GOLDEN).read().split('\n')
    assert want[-1] == '' and len(want) - 1 == 376
    assert have == sorted(want[:-1])


def test_outside_the_enumerated_ranges_there_is_no_kernel():
    for cell in ((0, 0, 0, 0, 0, 1), (9, 0, 0, 1, 0, 1), (1, -1, 0, 0, 0, 1), (1, 10, 1, 0, 0, 0), (1, 0, 3, 0, 0, 0), (1, 0, -1, 0, 0, 0),
                 (1, 0, 0, 4, 0, 1), (1, 0, 0, -1, 0, 1), (1, 0, 0, 0, 0, 3), (1, 0, 0, 0, 0, -1)):
        found, listed = C.c_int32(-1), C.c_int32(-1)
        assert _lib.lib().tsem_debug_fused_cell(*cell, C.byref(found), C.byref(listed)) == _lib.OK
        assert (found.value, listed.value) == (0, 0), cell
