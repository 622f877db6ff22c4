"""`-m gpu`: layouts that FILL the fused kernel's LDS, against the exact reference of tests/_em_pass_reference.py.

The kernel takes its twelve LDS regions from one map (csrc/tsem_fused_lds.h) and the host sizes the launch, the row slots and the
log-Q table from the same map; tests/test_fused_lds_host.py shows on the host that the regions are disjoint and inside the launch.
Here the device runs where a wrong map would corrupt a neighbouring table: every layout class at its largest part (TS_MAX_KP 7680,
TS_MAX_KP_LNL 5120, TS_MAX_KP3 4800, the split layout's 15 360 columns), a 2048-entry score table in LDS, the row slots left to
the library — which takes the most the set-up gives such a layout: tsem_debug_fused_lds' rmax, cut to a multiple of 8, asserted —
and again forced past the reserve the set-up keeps, to the last multiple of 8 the launch check admits (less than one row slot's
bytes stay free).  The lnl pass's log-Q table takes what the room leaves.  Score codes and fp64 entries where the class has both.

Each leg asserts that layout_info's lds_bytes is what the map says for that layout, that the layout is a fused one, and checks 1 - 4
of the exact ladder (tests/test_gpu_em_pass_exact.py: column sums, the lnl pass in the forms fused_dbg 0 / 8192 / 32768 where the
layout has them, the update bit for bit, the passes after it) with its bounds unchanged; the use_likelihood leg runs the carrying
pass (MODE 4: three tables and the rp ring) the way tests/test_gpu_fused_cells.py does.  The matrices are `ring` / `short` rows
over as many columns as the class's part holds: some 10 000 rows, so a dozen teams walk one or two blocks each — every region is
loaded and used; the steady state of the pipeline is tests/test_gpu_fused_cells.py's subject.

The last test asks for more row slots than fit: the host answers (layout_decide_format), first by keeping the score table out of
LDS, then by falling back to the two-pass kernels, and the results are the reference's.  Nothing past the limit is attempted on the
device."""
import numpy as np
import pytest

import _em_pass_reference as E
from test_fused_lds_host import CLASSES, CODES, FZ_RMAX, LDS_DYN_MAX, lds
from test_gpu_em_pass_exact import Model, _leg
from test_gpu_em_pass_exact import _nothing_after_a_fault  # noqa: F401  (the fault latch: an autouse fixture)
from test_gpu_fused_cells import _carried_lnl

pytestmark = pytest.mark.gpu
ROWS = 10000
_matrices = {}


def _say(fmt, *a):
    print('FUSEDLDSFULL ' + fmt % a, flush=True)


def _lut2048(raw):
    """the model's table behind 2048 entries: the largest score table that goes into LDS"""
    t = E.lut(raw)
    return np.concatenate([t, np.repeat(t[-1], 2048 - len(t))])


def _matrix(short, K):
    key = ('lds_short' if short else 'lds_ring', K)
    if key not in _matrices:
        _matrices[key] = E.short_row_matrix(ROWS, K) if short else E.ring_matrix(ROWS, K)
    return _matrices[key], key


# name, layout class (tests/test_fused_lds_host.py), parts, geometry, columns (K / parts + the 64 hot-column slots = the class's part),
# extra options
LAYOUTS = (
    ('two-tables-g2', 'plain', 1, 2, 7616, ()),
    ('two-tables-g3', 'plain', 1, 3, 7616, ()),
    ('use_likelihood', 'use_likelihood', 1, 2, 5056, (('use_likelihood', 1),)),
    ('reproducible1', 'reproducible1', 1, 2, 4736, (('reproducible', 1),)),
    ('reproducible2', 'reproducible2', 1, 2, 7616, (('reproducible', 2),)),
    ('split', 'split', 5, 2, 5 * 15296, (('split', 1),)),
)
FORMATS = {'plain': (1, 2), 'use_likelihood': (1,), 'reproducible1': (1,), 'reproducible2': (1, 2), 'split': (1, 2)}
LEGS = [(name, cls, P, geo, K, extra, fmt, forced) for (name, cls, P, geo, K, extra) in LAYOUTS for fmt in FORMATS[cls] for forced in (False, True)]


def _options(P, geo, extra, fmt, block_rows=None):
    o = (('parts', P), ('geometry', geo), ('value_format', 2 if fmt == 1 else 1)) + extra
    return o + ((('block_rows', block_rows),) if block_rows else ())


def _host(cls, geo, Kp, R, fmt):
    """(lds_bytes, rmax, room) of such a layout, from the map"""
    return lds((1, 0, 0, geo, 0, 1), Kp, R, 2048, 0, 0, CLASSES[cls][0] | (CODES if fmt else 0), regions=False)[2:]


@pytest.mark.parametrize('name,cls,P,geo,K,extra,fmt,forced', LEGS, ids=lambda v: str(v) if not isinstance(v, tuple) else '')
def test_full_lds(gpu_device, name, cls, P, geo, K, extra, fmt, forced):
    Kp = CLASSES[cls][1]
    assert -(-K // P) + 64 == Kp
    rmax = _host(cls, geo, Kp, 64, fmt)[1]
    assert 64 <= rmax <= FZ_RMAX[geo]
    raw, mkey = _matrix(geo == 3, K)
    label = '%s-f%d-%s' % (name, fmt, 'edge' if forced else 'auto')
    edge = rmax // 8 * 8                                   # forced: the last multiple of 8 the host's launch check admits
    while edge + 8 <= FZ_RMAX[geo] and _host(cls, geo, Kp, edge + 8, fmt)[0] <= LDS_DYN_MAX:
        edge += 8
    m = Model(gpu_device, raw, _options(P, geo, extra, fmt, edge if forced else None), lut=_lut2048(raw))
    info = m.info = m.eng.layout_info(extended=True)
    want, _, room = _host(cls, geo, info['Kp'], info['R'], fmt)
    _say('%s: P %d Kp %d R %d (rmax %d) nb %d geometry %d lds_bytes %d of %d, room for log Q %d B', label, info['P'], info['Kp'], info['R'], rmax,
         info['nb'], info['geometry'], info['lds_bytes'], LDS_DYN_MAX, room)
    assert info['fused'] == 1 and info['P'] == P and info['Kp'] == Kp and info['geometry'] == geo and info['value_bytes'] == (2 if fmt == 1 else 8), info
    assert info['split'] == (1 if cls == 'split' else 0) and info['lnl_fused'] == (1 if cls == 'use_likelihood' else 0), info
    assert info['exact_single'] == (1 if cls == 'reproducible1' else 0), info
    assert info['lds_bytes'] == want <= LDS_DYN_MAX, (info, want)
    assert info['R'] == (edge if forced else rmax // 8 * 8), (info, rmax, edge)
    if cls == 'use_likelihood':
        top = _carried_lnl(m, mkey, label)
    else:
        repro = cls in ('reproducible1', 'reproducible2')
        top = _leg(m, mkey, ('decades',), label, forms=(0, 8192, 32768) if cls == 'plain' else (0,), limit_of=E.repro_limit if repro else None)
    after = m.eng.layout_info(extended=True)
    _say('%s: lnl_tables %d lnl_linear %d | largest: column sums %.3f lnl %.3g diff %.3f', label, after['lnl_tables'], after['lnl_linear'], top[0], top[1], top[2])
    assert after['fallbacks'] == 0 and after['fused'] == 1, after
    if cls == 'plain':                                     # the log-Q table goes into the room the map leaves, or nowhere
        assert after['lnl_linear'] == 0 and after['lnl_tables'] * 8 <= room, (after, room)
        if fmt == 1:                                       # (score codes: one entry per code, all of them or none)
            assert after['lnl_tables'] == (2048 if 2048 * 8 <= room else 0), (after, room)


def test_the_log_q_table_fills_the_room(gpu_device):
    """MODE 9 at the limit: 7680 columns, score codes, and the most row slots that still leave the room for the 2048 entries of log Q
    (the table is not the reference's arithmetic one, so the look-up table it is) — lq and the log table behind it end within one row
    slot's bytes of the limit"""
    cls, geo, K, fmt = 'plain', 2, 7616, 1
    Kp = CLASSES[cls][1]
    R = 64
    while _host(cls, geo, Kp, R + 8, fmt)[2] >= 2048 * 8:
        R += 8
    room = _host(cls, geo, Kp, R, fmt)[2]
    assert 2048 * 8 <= room < 2048 * 8 + 8 * 48 and R < _host(cls, geo, Kp, 64, fmt)[1]
    launch = lds((1, 9, fmt, geo, 0, 0), Kp, R, 2048, 2048, 0, CODES, regions=False)[2]
    assert LDS_DYN_MAX - 8 * 48 < launch <= LDS_DYN_MAX
    raw, mkey = _matrix(False, K)
    m = Model(gpu_device, raw, _options(1, geo, (), fmt, R), lut=_lut2048(raw))
    info = m.info = m.eng.layout_info(extended=True)
    assert info['fused'] == 1 and info['R'] == R and info['Kp'] == Kp and info['value_bytes'] == 2, info
    top = _leg(m, mkey, ('decades',), 'log-q-full', forms=(0, 8192, 16384 | 32768, 32768))
    after = m.eng.layout_info(extended=True)
    _say('log-q-full: R %d lds_bytes %d + log Q %d B = %d of %d | lnl_tables %d lnl_linear %d | largest: column sums %.3f lnl %.3g', R, info['lds_bytes'],
         2048 * 8, launch, LDS_DYN_MAX, after['lnl_tables'], after['lnl_linear'], top[0], top[1])
    assert after['lnl_tables'] == 2048 and after['lnl_linear'] == 0 and after['fallbacks'] == 0, after
    ran = {c for c, (n, _) in m.eng.fused_launches().items() if n > 0}
    assert (1, 9, 1, geo, 0, 0) in ran, sorted(ran)


def test_more_row_slots_than_fit_are_answered_on_the_host(gpu_device):
    """block_rows past what the LDS holds, at 7680 columns with fp64 entries.  The set-up's rmax keeps a reserve below the launch check,
    so rmax + 8 is still a fused layout with the score table in LDS.  The first multiple of 8 whose launch bytes exceed the limit WITH
    the score table is answered by layout_decide_format: the layout stays fused and the table stays out of LDS (fp64 row weights),
    launched with what the map says without it.  Without the table 7680 columns leave room for more row slots than geometry 2 has, so
    the next refusal is the geometry's: fz_rmax + 8 falls back to the two-pass kernels.  Both are host decisions, both give the
    reference's results; nothing past the limit is launched."""
    cls, geo, K = 'plain', 2, 7616
    Kp = CLASSES[cls][1]
    rmax = _host(cls, geo, Kp, 64, 2)[1]
    assert _host(cls, geo, Kp, rmax // 8 * 8 + 8, 2)[0] <= LDS_DYN_MAX
    R = rmax // 8 * 8 + 8
    while _host(cls, geo, Kp, R, 2)[0] <= LDS_DYN_MAX:
        R += 8
    assert R <= FZ_RMAX[geo] and _host(cls, geo, Kp, R, 0)[0] <= LDS_DYN_MAX
    raw, mkey = _matrix(False, K)
    for rows, fused in ((R, 1), (FZ_RMAX[geo] + 8, 0)):
        m = Model(gpu_device, raw, _options(1, geo, (), 2, rows), lut=_lut2048(raw))
        info = m.info = m.eng.layout_info(extended=True)
        _say('block_rows %d (rmax %d): fused %d R %d lds_bytes %d lnl_tables %d', rows, rmax, info['fused'], info['R'], info['lds_bytes'], info['lnl_tables'])
        assert info['fused'] == fused and info['R'] == rows and info['value_bytes'] == 8, info
        assert info['lds_bytes'] == (_host(cls, geo, Kp, rows, 0)[0] if fused else 0), info
        _leg(m, mkey, ('decades',), 'block_rows-%d' % rows, forms=(0, 8192) if fused else False)
        after = m.eng.layout_info(extended=True)
        assert after['fallbacks'] == 0 and after['lnl_tables'] == 0, after
