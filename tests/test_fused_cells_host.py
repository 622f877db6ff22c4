"""The plan of the fused-kernel sweep (tests/_fused_cells.py) against the committed list of instantiations
(tests/golden/fused_kernels.txt), on the host, no GPU: every one of the 376 kernels is named by a leg of
tests/test_gpu_fused_cells.py — which launches it against the exact reference and asserts from the launch census that it did — or
stands in UNREACHABLE with the host rule that keeps every option set from launching it.  A kernel added to the table has neither,
and this file fails until it has."""
import ctypes as C

import pytest

import _fused_cells as F
from telescope_amd import _lib
from test_fused_table_host import CELLS, GOLDEN


@pytest.fixture(scope='module')
def golden():
    lines = open(GOLDEN).read().split('\n')
    assert lines[-1] == '' and len(lines) - 1 == 376
    return set(lines[:-1])


def _planned():
    return set().union(*(leg.cells for leg in F.LEGS))


def test_every_kernel_has_a_leg_or_a_rule(golden):
    planned = {F.kernel_name(c) for c in _planned()}
    unreachable = {F.kernel_name(c) for c in F.UNREACHABLE}
    print('FUSEDCELLS plan: %d legs name %d cells; UNREACHABLE holds %d' % (len(F.LEGS), len(planned), len(unreachable)))
    assert planned & unreachable == set()
    assert sorted(golden - planned - unreachable) == [], 'kernels no leg launches'
    assert sorted((planned | unreachable) - golden) == [], 'cells outside the committed list'
    assert len(planned) + len(unreachable) == 376


def test_unreachable_entries_quote_their_rule():
    for cell, rule in F.UNREACHABLE.items():
        assert cell in CELLS and isinstance(rule, F.Rule) and ':' in rule.text and len(rule.text) > 40, (cell, rule)
        assert rule.lands is None or (rule.lands and cell not in rule.lands and set(rule.lands) <= _planned()), (cell, rule)
    assert len(F.UNREACHABLE) <= 8, 'more than a handful: the census has found dead instantiations — report them'


def test_legs_are_distinct_and_within_the_enumerated_ranges():
    names = [leg.name for leg in F.LEGS]
    assert len(set(names)) == len(names)
    options = [(leg.options, leg.big_lut) for leg in F.LEGS]
    assert len(set(options)) == len(options), 'two legs build the same layout'
    for leg in F.LEGS:
        assert leg.cells and leg.cells <= set(CELLS), leg
        assert leg.kind in F.KINDS and leg.matrix in ('ring', 'short4k'), leg
    # no cell is named by two legs: a mutation confined to one cell fails one leg
    counts = {}
    for leg in F.LEGS:
        for c in leg.cells:
            counts[c] = counts.get(c, 0) + 1
    assert [c for c, n in counts.items() if n != 1] == []


def test_every_leg_is_consistent_with_the_table():
    """the options of a leg, read the way the layout build reads them (the module's docstring), against every cell it names — and every
    such cell is a kernel that exists, by the look-up and by the predicate"""
    L = _lib.lib()
    for leg in F.LEGS:
        o = dict(leg.options)
        fmt = 1 if o['value_format'] == 2 else (0 if leg.big_lut else 2)
        split = o.get('split') == 1
        ix = 0 if (fmt == 1 or split) else o['index_format']
        assert o['geometry'] in ((1, 2) if o['parts'] > 4 else (0, 2, 3)), leg
        if ix == 2:
            assert o['geometry'] in (0, 1) and fmt != 1 and 'reproducible' not in o, leg      # (quad_possible, tsem_setup.hip)
        if split:
            assert o['parts'] > 4 and 'reproducible' not in o, leg
        if 'use_likelihood' in o:
            assert fmt == 1 and o['geometry'] != 3 and not split, leg                           # (lnl3_possible; geometry 3 falls to 0)
        if o.get('reproducible') == 1:
            assert fmt == 1, leg                                                                # (exact_single: not with value_format 1)
        if 'reproducible' in o:
            assert fmt != 0, leg
        prof = 1 if 'fused_prof' in o else 0
        for (P, mode, f, g, t, x) in leg.cells:
            assert (P, f, g, t, x) == (o['parts'], fmt, o['geometry'], prof, ix), (leg.name, (P, mode, f, g, t, x))
            assert mode in F.MODES[leg.kind], (leg.name, mode)
            found, listed = C.c_int32(-1), C.c_int32(-1)
            assert L.tsem_debug_fused_cell(P, mode, f, g, t, x, C.byref(found), C.byref(listed)) == _lib.OK
            assert (found.value, listed.value) == (1, 1), (leg.name, (P, mode, f, g, t, x))
        # ... and the leg names EVERY kernel that exists for its layout in the modes its passes launch
        for mode in F.MODES[leg.kind]:
            found, listed = C.c_int32(-1), C.c_int32(-1)
            assert L.tsem_debug_fused_cell(o['parts'], mode, fmt, o['geometry'], prof, ix, C.byref(found), C.byref(listed)) == _lib.OK
            assert ((o['parts'], mode, fmt, o['geometry'], prof, ix) in leg.cells) == bool(found.value), (leg.name, mode)


def test_census_entry_points_are_declared_and_refuse_null():
    for name in ('tsem_debug_fused_launches', 'tsem_debug_fused_launches_clear'):
        assert name in _lib.exported_symbols() and hasattr(_lib.lib(), name)
    assert _lib.lib().tsem_debug_fused_launches(None, None, 0) == _lib.ERR_ARG
    assert _lib.lib().tsem_debug_fused_launches_clear(None) == _lib.ERR_ARG
    assert len(CELLS) == 5760


def test_the_census_order_is_one_order():
    """_lib.FUSED_CELLS (what fused_launches() names its counters by), the table test's CELLS and the library's fz_census_cell"""
    assert _lib.FUSED_CELLS == CELLS
    L = _lib.lib()
    assert [L.tsem_debug_fused_census_index(*c) for c in CELLS] == list(range(len(CELLS)))
    for outside in ((0, 0, 0, 0, 0, 0), (9, 0, 0, 0, 0, 0), (1, 10, 0, 0, 0, 0), (1, 0, 3, 0, 0, 0), (1, 0, 0, 4, 0, 0), (1, 0, 0, 0, 0, 3)):
        assert L.tsem_debug_fused_census_index(*outside) == -1, outside


def test_the_row_shape_legs_are_twins_of_planned_legs():
    by_name = {leg.name: leg for leg in F.LEGS}
    assert len(F.SHAPE_LEGS) == sum(1 for leg in F.LEGS if leg.P in (4, 8)) > 0
    for leg in F.SHAPE_LEGS:
        twin = by_name[leg.name[len('shape-'):]]
        assert leg.cells == twin.cells and leg.matrix == 'row_shape' and 'block_rows' not in dict(leg.options), leg
        assert dict(leg.options) == {k: v for k, v in twin.options if k != 'block_rows'}, leg
    families = {(leg.kind, leg.geo, leg.fmt, leg.ix, leg.P > 4) for leg in F.LEGS}
    assert families == {(leg.kind, leg.geo, leg.fmt, leg.ix, leg.P > 4) for leg in F.SHAPE_LEGS}


def _with(d, key, value):
    out = dict(d)
    out[key] = value
    return out


def test_assert_census_fails_when_it_should():
    """the assertion every GPU leg ends with, on made-up census values: equal passes; a neighbouring cell, a missing cell, a cell that
    was only launched conditionally, a fall-back, another index format and a `reproducible` that gave up each fail"""
    leg = next(l for l in F.LEGS if l.name == 'plain-P6-g1-f2-x1')
    repro = next(l for l in F.LEGS if l.name == 'repro2-P3-g2-f1-x0')
    good = {c: (2, 0) for c in leg.cells}
    after = {'fallbacks': 0, 'index_format': leg.ix, 'reproducible': 0}
    F.assert_census(leg, good, after)
    F.assert_census(leg, _with(good, (6, 1, 2, 2, 0, 1), (0, 5)), after)                     # a neighbour launched conditionally only: no coverage, no failure
    one = sorted(leg.cells)[0]
    neighbour = (one[0], one[1], one[2], 2, one[4], one[5])                                     # the same kernel on geometry 2
    cases = [(leg, _with({c: v for c, v in good.items() if c != one}, neighbour, (2, 0)), after),
             (leg, _with(good, neighbour, (1, 0)), after),
             (leg, {c: v for c, v in good.items() if c != one}, after),
             (leg, _with(good, one, (0, 3)), after),
             (leg, good, dict(after, fallbacks=1)),
             (leg, good, dict(after, index_format=2)),
             (repro, {c: (9, 0) for c in repro.cells}, {'fallbacks': 0, 'index_format': repro.ix, 'reproducible': 3})]
    F.assert_census(repro, {c: (9, 0) for c in repro.cells}, {'fallbacks': 0, 'index_format': repro.ix, 'reproducible': 1})
    for lg, census, aft in cases:
        with pytest.raises(AssertionError):
            F.assert_census(lg, census, aft)


def test_every_gpu_leg_ends_with_the_census_assertion():
    """tests/test_gpu_fused_cells.py::_run — what both parametrised tests go through — calls assert_census, and returns nothing before it"""
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_fused_cells.py')).read()
    tree = ast.parse(src)
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef)}
    run = fns['_run']
    calls = [n for n in ast.walk(run) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and n.func.attr == 'assert_census']
    returns = [n for n in ast.walk(run) if isinstance(n, ast.Return)]
    assert len(calls) == 1 and len(returns) == 1
    assert returns[0] is run.body[-1] and calls[0].lineno < returns[0].lineno, 'a return in front of the census assertion'
    assert isinstance(run.body[-2], ast.Expr) and run.body[-2].value is calls[0], 'the assertion is not at the top level of _run'
    for name in ('test_cell', 'test_cell_on_row_shapes'):
        assert any(isinstance(n, ast.Call) and getattr(n.func, 'id', None) == '_run' for n in ast.walk(fns[name])), name
