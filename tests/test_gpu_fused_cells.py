"""`-m gpu`: EVERY instantiation of the fused kernel k_em_fused<P, MODE, FMT, GEO, PROF, IX> (the 376 lines of
tests/golden/fused_kernels.txt) against the exact reference of tests/_em_pass_reference.py, one leg of tests/_fused_cells.py per
layout.  A leg forces its layout, pins it from layout_info, runs the checks of the exact ladder (tests/test_gpu_em_pass_exact.py:
1 column sums, 2 every form of the lnl pass it names, 3 the update bit for bit, 4 the passes after the update) with the parameter
sets `decades` and `dying`, and then asserts from the launch census (`_lib.Engine.fused_launches`) that the kernels it launched
unconditionally are EXACTLY the cells it names — a leg that silently lands on a neighbouring kernel fails there.
tests/test_fused_cells_host.py shows without a GPU that the legs name every kernel.

The bounds are those of the reference, unchanged: functions of entry counts, row lengths and the path (FUSED with P, SPLIT), not of
the geometry, the format or the mode.  Per kind of leg:
  plain    checks 1 - 4 with every form of the lnl pass the layout has: MODE 0, 1 and 9;
  repro2 / repro1   option `reproducible` 2 / 1, checks 1 - 4 against E.repro_limit: MODE 2 / MODE 3;
  lnl4     the carried log-likelihood: two chunks of one iteration each with use_likelihood — the first pass carries nothing, the
           second sums the lnl of the first iteration next to its column sums —, check 1 on both passes' sums, check 3 on the first
           update, the carried value against the exact lnl within the limit of check 2: MODE 4;
  split    checks 1 - 4 on the forced split layout: MODE 5, 7 and 8;
  prof     the timeline kernel is an EM pass: check 1 and check 3.
Shapes.  test_cell: `ring` (2 - 12 entries per row over 4000 columns; geometry 3: `short4k`, 2 - 6 entries over the same columns) in
blocks of 64 rows, with as many rows as give EVERY team F.STEADY = 7 blocks to walk on the device at hand (F.rows_of from the CU
count: 141 000 rows for teams of 1 on 256 CUs, 17 700 for teams of 8; asserted from layout_info): every register set is refilled,
the offs ring, the y, s and rp rings and the exchange slots are reused — the pipeline's steady state, not only its prologue.  A
block of 64 such rows fills a small part of a register tile; test_cell_on_row_shapes therefore runs the teams of 4 and of 8 of every
family (kind, geometry, formats) again on the row-shape matrix with the block size left to the library: tiles filled to their
capacity, rows of 63 ... 1000 entries that cross waves, the row of K - 2.  Wrapping the rings TWICE stays test_rings_wrap_twice's
subject on the cells it reaches.

Prints `FUSEDCELLS ...` lines with every leg's largest fractions of its bounds (`pytest -s`); profiles/r36_fused_cells.txt keeps a
run, with the planted mutations and the legs each one failed."""
import time

import numpy as np
import pytest

import _em_pass_reference as E
import _fused_cells as F
from test_gpu_em_pass_exact import LD, Model, _check_pass, _check_red, _check_update, _leg, _ref
from test_gpu_em_pass_exact import cu_count  # noqa: F401  (a fixture)
from test_gpu_em_pass_exact import _nothing_after_a_fault  # noqa: F401  (the fault latch: an autouse fixture)
from test_gpu_quad64 import _big_lut

pytestmark = pytest.mark.gpu
SETS = ('decades', 'dying')


def _say(fmt, *a):
    print('FUSEDCELLS ' + fmt % a, flush=True)


_short4k = {}


def _matrix(name, rows):
    """(matrix, its key among the shared references)"""
    if name == 'row_shape':
        return E.matrix('row_shape'), 'row_shape'
    if name == 'short4k':
        if rows not in _short4k:
            _short4k[rows] = E.short_row_matrix(rows, 4000)
        return _short4k[rows], ('short4k', rows)
    return E.matrix(name, rows), (name, rows)


def _build(gpu_device, options, big_lut, name, rows):
    raw, mkey = _matrix(name, rows)
    m = Model(gpu_device, raw, options, lut=_big_lut(raw) if big_lut else None)
    m.info = m.eng.layout_info(extended=True)
    m.eng.clear_fused_launches()
    return m, mkey


def _unconditional(eng):
    return {c for c, (n, _) in eng.fused_launches().items() if n > 0}


def _carried_lnl(m, mkey, label):
    """MODE 4 (see the module's docstring); returns the largest fractions (column sums, lnl, diff_est)"""
    top = [0.0, 0.0, 0.0]
    P = m.path()[1]
    for pname in SETS:
        ref = _ref(mkey, m.raw, pname)
        lab = '%s/%s' % (label, pname)
        m.eng.set_params(ref.pi, ref.theta)
        m.eng.set_params(ref.pi, ref.theta)
        d1, l1, stopped = m.eng.em_chunk(1, 0.0, use_likelihood=True, first=True)
        assert len(d1) == 1 and not stopped and np.isnan(l1[0]) and np.isnan(m.eng.lnl_carry), (lab, d1, l1, stopped)
        f1, red = _check_red(m, ref, m.eng.read_reduce(0, m.K + 2), lab)
        df, pi_c, th_c, _, _ = _check_update(m, red, ref.pi, ref.theta, lab, diff=float(d1[0]))
        ref2 = E.PassReference(m.raw, m.lut, pi_c, th_c, ref.pi, ref.theta)
        assert ref2.fair == [], (lab, 'after the update', ref2.fair)
        d2, l2, stopped = m.eng.em_chunk(1, 0.0, use_likelihood=True, last=True)
        carry = m.eng.lnl_carry
        assert len(d2) == 1 and not stopped and np.isfinite(carry) and np.isfinite(l2[0]), (lab, d2, l2, carry)
        red2 = m.eng.read_reduce(0, m.K + 2)
        # (slots K and K + 1 hold log-likelihoods by now — the flush's dedicated pass sums into slot K, the carried value rode in slot
        # K + 1 —, so check 1 cannot read the time-out word of this pass there.  A time-out of a pass inside a chunk reaches the host
        # another way: the update commits nothing, em_chunk retries and counts it, and the fall-back it takes shows in layout_info —
        # len(d2) == 1 and not stopped above, and `fallbacks == 0` in assert_census, are this pass's time-out check.)
        assert np.all(np.isfinite(red2[m.K:])), (lab, red2[m.K:])
        f4, _ = _check_red(m, ref2, red2, lab + '/carrying pass', slots=False)
        lf = float(abs(LD(carry) - ref2.lnl) / ref2.lnl_limit_P(P))
        _say('%s: column sums %.3f, of the carrying pass %.3f of the bound; carried lnl %.3g of its limit; diff_est %.3f of its bound',
             lab, f1, f4, lf, df)
        assert lf <= 1.0, (lab, 'carried lnl', carry, float(ref2.lnl), lf)
        top = [max(top[0], f1, f4), max(top[1], lf), max(top[2], df)]
    return top


def _timeline(m, mkey, label):
    """PROF: check 1 and check 3"""
    top = [0.0, 0.0, 0.0]
    for pname in SETS:
        ref = _ref(mkey, m.raw, pname)
        lab = '%s/%s' % (label, pname)
        m.eng.set_params(ref.pi, ref.theta)
        m.eng.set_params(ref.pi, ref.theta)
        f1, red = _check_pass(m, ref, lab)
        df = _check_update(m, red, ref.pi, ref.theta, lab)[0]
        top = [max(top[0], f1), 0.0, max(top[2], df)]
    return top


def _run(gpu_device, leg, teams, rows):
    t0 = time.time()
    m, mkey = _build(gpu_device, leg.options, leg.big_lut, leg.matrix, rows)
    info = m.info
    for key, want in F.expected_layout(leg).items():
        assert info[key] == want, (leg.name, key, want, info)
    repro = leg.kind in ('repro1', 'repro2')
    assert (info['reproducible'] in (1, 2)) if repro else info['reproducible'] == 0, (leg.name, info)
    if rows:
        assert info['nb'] // teams >= F.STEADY, (leg.name, 'a team walks fewer than %d blocks: its pipeline never leaves the prologue' % F.STEADY, teams, info)
    if leg.kind == 'lnl4':
        top = _carried_lnl(m, mkey, leg.name)
    elif leg.kind == 'prof':
        top = _timeline(m, mkey, leg.name)
    else:
        top = _leg(m, mkey, SETS, leg.name, forms=leg.forms, limit_of=E.repro_limit if repro else None)
    census = m.eng.fused_launches()
    ran = {c for c, (n, _) in census.items() if n > 0}
    after = m.eng.layout_info(extended=True)
    _say('%s %s: rows %d P %d Kp %d R %d nb %d (>= %d per team of at most %d) max_subblock %d geometry %d value_bytes %d index_format %d split %d reproducible %d exact_single %d lnl_fused %d | '
         'cells %s | launches %d + %d conditional | largest: column sums %.3f lnl %.3g diff %.3f | %.2f s', leg.name, leg.matrix, m.raw.shape[0], info['P'],
         info['Kp'], info['R'], info['nb'], info['nb'] // teams, teams, info['max_subblock'], info['geometry'], info['value_bytes'], info['index_format'], info['split'], info['reproducible'],
         info['exact_single'], info['lnl_fused'], ' '.join(F.kernel_name(c) for c in sorted(ran)), sum(n for n, _ in census.values()),
         sum(c for _, c in census.values()), top[0], top[1], top[2], time.time() - t0)
    F.assert_census(leg, census, after)
    return info


@pytest.mark.parametrize('leg', F.LEGS, ids=lambda leg: leg.name)
def test_cell(gpu_device, cu_count, leg):  # noqa: F811
    teams, rows = F.rows_of(leg.P, cu_count)
    _run(gpu_device, leg, teams, rows)


@pytest.mark.parametrize('leg', F.SHAPE_LEGS, ids=lambda leg: leg.name)
def test_cell_on_row_shapes(gpu_device, cu_count, leg):  # noqa: F811
    """the row-shape matrix, the block size left to the library: the row of K - 2 entries cut over the parts sits in ONE sub-block of
    each, so a register tile holds at least (K - 2) / P entries of one row"""
    info = _run(gpu_device, leg, max(1, cu_count // leg.P), 0)
    assert -(-(6000 - 2) // leg.P) <= info['max_subblock'], (leg.name, info)


def test_unreachable_rules(gpu_device):
    """the host rule every UNREACHABLE entry quotes: forcing the options yields an error, or the passes land on other, named cells"""
    from telescope_amd import _lib
    _say('UNREACHABLE holds %d cells', len(F.UNREACHABLE))
    for cell, rule in sorted(F.UNREACHABLE.items()):
        if rule.lands is None:
            with pytest.raises(_lib.EngineError):
                _build(gpu_device, rule.options, rule.big_lut, 'ring', 3000)
            continue
        m, mkey = _build(gpu_device, rule.options, rule.big_lut, 'ring', 3000)
        _leg(m, mkey, ('decades',), 'unreachable-' + F.kernel_name(cell), forms=(0, 8192, 32768))
        ran = _unconditional(m.eng)
        assert cell not in ran and ran == set(rule.lands), (cell, sorted(ran))
