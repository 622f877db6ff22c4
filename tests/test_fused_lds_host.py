"""The fused kernel's LDS map (csrc/tsem_fused_lds.h) through tsem_debug_fused_lds, on the host, no GPU.

1. tests/golden/fused_lds.txt holds what the host computed BEFORE the map existed — three hand-written formulas: the bytes a layout's
   fused launches ask for (layout_info 'lds_bytes'), the most row slots tsem_choose_geometry gives it, and the room the log-Q table may
   take — recorded from the parent commit over layout class x geometry x Kp x R x lut_len x score table in LDS.  The map returns the
   same three numbers on every line.
2. What the copies never had: for every one of the 376 kernels and every point of that grid its layout class admits, the regions the
   KERNEL takes from the map are pairwise disjoint and aligned, and end within the bytes the HOST launches that kernel with, which are
   within the limit — MODE 9 with the largest log-Q table the room allows, and with the arithmetic log Q.  The checker rejects a
   hand-made map whose region is one element too long."""
import ctypes as C
import os

import pytest

from telescope_amd import _lib
from test_fused_table_host import GOLDEN as KERNELS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'fused_lds.txt')
LDS_DYN_MAX = 160 * 1024 - 1024                   # TS_LDS_DYN_MAX, tsem_common.h
SPLIT, EXACT_SINGLE, LNL3, REPRODUCIBLE, CODES = 1, 2, 4, 8, 16
# layout class: flags, the largest Kp (TS_MAX_KP, TS_MAX_KP_LNL, TS_MAX_KP3, TS_MAX_KP, 2 * TS_MAX_KP)
CLASSES = {'plain': (0, 7680), 'use_likelihood': (LNL3, 5120), 'reproducible1': (EXACT_SINGLE | REPRODUCIBLE, 4800),
           'reproducible2': (REPRODUCIBLE, 7680), 'split': (SPLIT, 15360)}
FZ_RMAX = {0: 512, 1: 384, 2: 768, 3: 1152}
ROWS = (64, 384, 512, 768, 1152)
REGIONS = ('c', 'acc', 'acc2', 'y', 's', 'rp', 'ibox', 'offs', 'dum', 'lut', 'lq', 'exps', 'logtab')


def lds(cell, Kp, R, lut_len, lq_n, lq_lin, flags, regions=True):
    """(regions {name: (offset, bytes)} or None, kernel_end, launch_bytes, rmax, room)"""
    reg = (C.c_int32 * 26)()
    out = [C.c_int32(-1) for _ in range(4)]
    rc = _lib.lib().tsem_debug_fused_lds(*cell, Kp, R, lut_len, lq_n, lq_lin, flags, reg if regions else None, *[C.byref(o) for o in out])
    assert rc == _lib.OK, (cell, Kp, R, lut_len, lq_n, lq_lin, flags)
    return ({n: (reg[2 * i], reg[2 * i + 1]) for i, n in enumerate(REGIONS)} if regions else None,) + tuple(o.value for o in out)


def check_map(regions, kernel_end, launch_bytes):
    """the property: every region the launch uses is 8-byte aligned (logtab 16), no two overlap, all end within the launch's bytes, and
    those within the limit"""
    live = sorted((at, at + n, name) for name, (at, n) in regions.items() if n > 0)
    for at, end, name in live:
        assert at >= 0 and at % (16 if name == 'logtab' else 8) == 0, (name, at)
        assert end <= kernel_end, (name, end, kernel_end)
    for (a0, a1, an), (b0, b1, bn) in zip(live, live[1:]):
        assert a1 <= b0, ('overlap', an, (a0, a1), bn, (b0, b1))
    assert kernel_end <= launch_bytes <= LDS_DYN_MAX, (kernel_end, launch_bytes)


def test_entry_point_is_declared_and_refuses_null():
    assert 'tsem_debug_fused_lds' in _lib.exported_symbols() and hasattr(_lib.lib(), 'tsem_debug_fused_lds')
    o = C.c_int32(0)
    assert _lib.lib().tsem_debug_fused_lds(1, 0, 0, 0, 0, 1, 64, 64, 0, 0, 0, 0, None, None, C.byref(o), C.byref(o), C.byref(o)) == _lib.ERR_ARG
    reg = (C.c_int32 * 26)()        # a cell outside the table has no map
    assert _lib.lib().tsem_debug_fused_lds(1, 4, 0, 0, 0, 0, 64, 64, 0, 0, 0, 0, reg, *[C.byref(o)] * 4) == _lib.ERR_ARG


def test_the_parents_numbers():
    lines = open(GOLDEN).read().split('\n')
    assert lines[-1] == '' and len(lines) - 1 == 2240
    seen = set()
    for ln in lines[:-1]:
        name, *v = ln.split()
        geo, Kp, R, lut_len, codes, lds_bytes, rmax, room = map(int, v)
        seen.add((name, geo))
        assert R <= FZ_RMAX[geo] and Kp <= CLASSES[name][1]
        _, _, got_bytes, got_rmax, got_room = lds((1, 0, 0, geo, 0, 1), Kp, R, lut_len, 0, 0, CLASSES[name][0] | (CODES if codes else 0), regions=False)
        assert (got_bytes, got_rmax, got_room) == (lds_bytes, rmax, room), ln
    assert seen == {(n, g) for n in CLASSES for g in range(4)}


def _classes_of(cell):
    """the layout classes that launch a cell (tests/_fused_cells.py: how the options reach a cell)"""
    P, mode, fmt, geo, prof, ix = cell
    out = []
    if mode in (0, 1, 9):
        out.append('plain')
    if mode in (0, 1, 4, 9) and fmt == 1 and geo != 3 and not prof:
        out.append('use_likelihood')
    if mode in (1, 3, 9) and fmt == 1:
        out.append('reproducible1')
    if mode in (1, 2, 9) and fmt != 0:
        out.append('reproducible2')
    if mode in (5, 7, 8):
        out.append('split')
    return out


def _cells():
    import re
    cells = []
    for ln in open(KERNELS).read().split('\n')[:-1]:
        P, mode, fmt, geo, prof, ix = re.match(r'k_em_fused<(\d), (\d), (\d), (\d), (true|false), (\d)>$', ln).groups()
        cells.append((int(P), int(mode), int(fmt), int(geo), 1 if prof == 'true' else 0, int(ix)))
    assert len(cells) == 376
    return cells


def test_every_kernel_stays_inside_what_the_host_launches():
    points = full = 0
    for cell in _cells():
        mode, fmt, geo = cell[1], cell[2], cell[3]
        names = _classes_of(cell)
        assert names, cell
        n_cell = 0
        for name in names:
            flags, kmax = CLASSES[name]
            for Kp in (64, 1000, kmax - 64, kmax):
                rmax = lds(cell, Kp, 64, 2048, 0, 0, flags, regions=False)[3]
                for R in sorted(set(r for r in ROWS if r <= FZ_RMAX[geo]) | ({rmax // 8 * 8} if rmax >= 64 else set())):
                    for lut_len in ((0, 200, 2048, 3000) if fmt == 0 else (200, 2048)):
                        fl = flags | (CODES if fmt != 0 else 0)
                        launch0 = lds(cell, Kp, R, lut_len, 0, 0, fl, regions=False)[2]
                        if launch0 > LDS_DYN_MAX:        # the host's own check (layout_decide_format): no fused layout of this size
                            continue
                        forms = [(0, 0)]
                        if mode == 9:
                            room = lds(cell, Kp, R, lut_len, 0, 0, fl, regions=False)[4]
                            assert room == LDS_DYN_MAX - launch0
                            forms = [(room // 8, 0)] + ([(lut_len, 1)] if fmt == 1 else [])
                        for lq_n, lq_lin in forms:
                            reg, kend, launch, _, _ = lds(cell, Kp, R, lut_len, lq_n, lq_lin, fl)
                            check_map(reg, kend, launch)
                            if mode == 9:
                                assert reg['lq'][1] == (0 if lq_lin else lq_n * 8) and launch == launch0 + reg['lq'][1]
                            points += 1
                            n_cell += 1
                            full += launch > LDS_DYN_MAX - 8 * 64
        assert n_cell >= 8, (cell, n_cell)
    print('FUSEDLDS %d points checked, %d of them within 512 B of the limit' % (points, full))
    assert full >= 376


def test_the_limits_are_what_the_map_leaves():
    """TS_MAX_KP / TS_MAX_KP_LNL / TS_MAX_KP3 / the split layout's part: at 64 row slots and a 2048-entry score table the layout fits
    the limit, and the set-up's own choice of R (rmax, with its reserve) still has 64 row slots, on every geometry"""
    for name, (flags, kmax) in CLASSES.items():
        for geo in range(4):
            launch, rmax = lds((1, 0, 0, geo, 0, 1), kmax, 64, 2048, 0, 0, flags | CODES, regions=False)[2:4]
            assert launch <= LDS_DYN_MAX and rmax >= 64, (name, geo, launch, rmax)


def test_the_checker_can_fail():
    cell = (4, 9, 1, 2, 0, 0)
    reg, kend, launch, _, _ = lds(cell, 7000, 512, 2048, 100, 0, CODES)
    check_map(reg, kend, launch)
    for name in ('acc', 's', 'dum', 'lut', 'lq'):           # one element too long: runs into its neighbour
        bad = dict(reg)
        bad[name] = (reg[name][0], reg[name][1] + 8)
        with pytest.raises(AssertionError):
            check_map(bad, kend, launch)
    bad = dict(reg)
    bad['logtab'] = (reg['logtab'][0] + 8, reg['logtab'][1])  # off its 16-byte boundary
    with pytest.raises(AssertionError):
        check_map(bad, kend + 8, launch)
    with pytest.raises(AssertionError):
        check_map(reg, kend, kend - 8)                         # the host launches with less than the kernel uses
    with pytest.raises(AssertionError):
        check_map(reg, kend, LDS_DYN_MAX + 8)
