"""`-m gpu`: EVERY iteration of the per-group EM fits (tsem_cell_em of telescope_amd/csrc/tsem_cellem.hip) — a wave per cell, 256
threads, 512 threads with the tables in LDS, 512 threads with the tables in the global workspace, and the spread class with its
three column tiers — against tests/_group_pass_reference.py: an exact (long double) reference of one step with rounding bounds that
are functions of counts, tied down without a GPU by tests/test_group_pass_reference.py.

The method: chained single steps, no new entry point.  For each leg `Engine.cell_em(eps, t, use_likelihood)` runs for t = 1 .. T on
one handle, driven through the C ABI alone (load_scores, max_score, rowstats, set_model, set_groups).  The unit is deterministic, so
run t repeats run t - 1 bit for bit and adds one iteration: what run t returns is checked against the reference evaluated on the
DEVICE'S OWN state of run t - 1.  No rounding error is carried from step to step.

Per leg and step t, for every group (`_run`):
 1. n_iter == min(t, the step it stopped at); converged == (|lnl_t - lnl_{t-1}| < eps) in fp64 on the device's own two numbers under
    use_likelihood, == (exact diff < eps) otherwise; col_ptr / cols are the group's distinct columns;
 2. z_t (export_z(Z_USER)): the pattern is the reference's — NaN outside it, NaN for rows in no group, no entry for a group whose
    reference z is NaN — and every stored value is within its bound;
 3. pi_t, theta_t, rest[0:2] within their bounds on every touched column, exact zeros exactly 0, NaN only where the reference has NaN;
 4. lnl_t within its limit;
 5. bitwise: pi_init, theta_init, rest[2:4] of run t equal pi, theta, rest[0:2] of run 1; a group that stopped at t* returns the same
    bits in every array, and the same z, for every max_iter > t* (the frozen-group path of k_sp_finish); twins inside a group have
    bit-identical pi and theta;
 6. layout_info reports the classes the case forces.
The conditions on the inputs (fair steps, stop margins, the extreme states met, a stopping and a non-stopping group per stopping
leg, a stop before, at and after the host's look in the spread class) are asserted from the reference's numbers on the device's
trajectory: they fail, they never skip.  No row, column, group or step is left out.  The legs print `GROUPPASS ...` lines with the
figures they assert on (`pytest -s`); profiles/r31_group_pass_exact.txt keeps a run.

Planted mutations of tsem_cellem.hip (each planted once in a scratch build, one line, never committed; profiles/r31_group_pass_exact.txt
section 3): the final ce_row_lnl writing z instead of NaN outside the pattern; the final lnl pass taking z from the current
parameters; k_sp_finish copying current -> previous for a group that stops as well; ce_col_sum dropping terms below 1e-30; theta
rounded to float in the E-step's product; a column's last term lost when below 1e-10 of the sum; theta from s (1 + 1e-10) — all
fail here; the last one passes the unit's three other GPU files."""
import numpy as np
import pytest

import _em_pass_reference as E
import _group_em_reference as G
import _group_pass_reference as P

pytestmark = pytest.mark.gpu
CLASS_NAMES = ('cell_em_wave', 'cell_em_256', 'cell_em_512', 'cell_em_global', 'cell_em_spread')
COLUMN_ARRAYS = ('pi', 'theta', 'pi_init', 'theta_init')
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


def _say(fmt, *a):
    print('GROUPPASS ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _engine(gpu_device):
    """an _lib.Engine that remembers a HIP error (TSEM_ERR_HIP, TSEM_ERR_TIMEOUT) for the fixture above"""
    from telescope_amd import _lib

    class Engine(_lib.Engine):
        def _ck(self, rc):
            if rc in (-2, -4):
                _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
            _lib.Engine._ck(self, rc)
    return Engine(gpu_device)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


class Dev(object):
    """An engine holding a case's matrix, model and group map, set through the C ABI alone."""

    def __init__(self, gpu_device, cs, priors):
        self.cs = cs
        self.eng = eng = _engine(gpu_device)
        eng.set_option('cell_em_spread_entries', cs.spread)
        raw = cs.raw
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), cs.K, cs.lut)
        eng.max_score()
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, *priors)
        eng.set_groups(cs.cor, cs.n_groups)

    def run(self, eps, max_iter, use_lnl):
        from telescope_amd import _lib
        r = self.eng.cell_em(eps, max_iter, use_lnl)
        z = self.eng.export_z(_lib.Z_USER)
        assert not np.any(np.isnan(z)) and np.all((z >= 0) | (z == -1.0)), 'tsem_export_z: a value that is neither a z nor the mark -1'
        r['z'] = np.where(z == -1.0, np.nan, z)                 # tsem_export_z marks `no entry` (NaN in the Z_USER buffer) with -1
        info = self.eng.layout_info()
        r['classes'] = tuple(int(info[n]) for n in CLASS_NAMES)
        return r

    def close(self):
        self.eng.close()


def _group_result(r, g):
    """what run `r` returned for group g: the column arrays on its columns, its scalars, its z"""
    a, b = int(r['col_ptr'][g.c]), int(r['col_ptr'][g.c + 1])
    out = {name: r[name][a:b].copy() for name in COLUMN_ARRAYS}
    out.update(rest=r['rest'][g.c].copy(), lnl=float(r['lnl'][g.c]), n_iter=int(r['n_iter'][g.c]), converged=int(r['converged'][g.c]),
               z=r['z'][g.ent].copy(), cols=r['cols'][a:b].copy())
    out['rest_pi'], out['rest_th'] = float(out['rest'][0]), float(out['rest'][1])
    return out


def _same_result(a, b):
    """the names of the arrays of two group results that differ in a bit"""
    return [k for k in COLUMN_ARRAYS + ('rest', 'z', 'lnl') if not np.array_equal(_bits(a[k]), _bits(b[k]))] + \
           [k for k in ('n_iter', 'converged') if a[k] != b[k]]


def _run(gpu_device, cs, priors, use_lnl, eps, label):
    """runs t = 1 .. T of one leg with checks 1 - 6; returns (worst fractions, the step every group stopped at, the extreme states
    met per group)"""
    d = Dev(gpu_device, cs, priors)
    groups = cs.groups()
    worst, stopped, frozen, flags, first, prev = {}, {}, {}, {}, {}, {}
    no_group = np.repeat(cs.cor < 0, np.diff(cs.raw.indptr))
    twins = {g.c: g.twin_classes() for g in groups}
    try:
        for t in range(1, cs.T + 1):
            r = d.run(eps, t, use_lnl)
            assert r['classes'] == cs.class_counts(), (label, t, 'layout_info', r['classes'], cs.class_counts())                 # 6
            assert len(r['col_ptr']) == cs.n_groups + 1 and r['col_ptr'][0] == 0 and r['col_ptr'][-1] == len(r['cols'])
            assert np.all(np.isnan(r['z'][no_group])), (label, t, 'rows in no group have entries in z')                          # 2
            for g in groups:
                tag = (label, 'group', g.c, 'step', t)
                got = _group_result(r, g)
                assert np.array_equal(got['cols'], g.cols), tag + ('cols',)                                                      # 1
                if len(g.rows) == 0:                                            # a group without rows is not fitted
                    assert got['n_iter'] == 0 and got['converged'] == 0 and np.isnan(got['lnl']), tag
                    assert got['rest'][0] == got['rest'][1] == 1.0 / cs.K and np.all(np.isnan(got['rest'][2:])), tag
                    continue
                if g.c in stopped:                                              # 5: frozen since t*
                    assert got['n_iter'] == stopped[g.c] and got['converged'] == 1, tag + ('n_iter', got['n_iter'], stopped[g.c])
                    assert _same_result(got, frozen[g.c]) == [], tag + ('differs from the run it stopped in', _same_result(got, frozen[g.c]))
                    continue
                if t == 1:
                    pi_prev, th_prev = g.start()
                    lnl_prev = np.inf
                    first[g.c] = got
                else:
                    p = prev[g.c]
                    pi_prev, th_prev, lnl_prev = g.dense(p['pi'], p['rest_pi']), g.dense(p['theta'], p['rest_th']), p['lnl']
                st = P.Step(g, priors, pi_prev, th_prev)
                assert st.fair == [], tag + ('the reference calls this step unfair', st.fair)
                P.check_step(st, got, worst, tag)                                                                                # 2, 3, 4
                f = flags.setdefault(g.c, dict(zero=0, gradual=0, left=0))
                for k in f:
                    f[k] += int(st.flags[k])
                with np.errstate(invalid='ignore'):
                    x = abs(np.float64(got['lnl']) - np.float64(lnl_prev)) if use_lnl else float(st.diff(g.dense(got['pi'], got['rest_pi'])))
                assert E.fair_stops([x], eps) == [], tag + ('the stop test lies within 1e-6 of epsilon', x, eps)
                want = bool(x < eps)
                assert got['n_iter'] == t and got['converged'] == int(want), tag + ('n_iter / converged', got['n_iter'], got['converged'], x, eps)   # 1
                for a, b in (('pi_init', 'pi'), ('theta_init', 'theta')):                                                       # 5
                    assert np.array_equal(_bits(got[a]), _bits(first[g.c][b])), tag + (a, 'is not run 1\'s', b)
                assert np.array_equal(_bits(got['rest'][2:]), _bits(first[g.c]['rest'][:2])), tag + ('rest[2:4] is not run 1\'s rest[0:2]',)
                for cls in twins[g.c]:
                    j = np.searchsorted(g.cols, cls)
                    for name in ('pi', 'theta'):
                        assert len(set(_bits(got[name][j]).tolist())) == 1, tag + ('twins differ in', name, cls)
                if want:
                    stopped[g.c], frozen[g.c] = t, got
                prev[g.c] = got
    finally:
        d.close()
    return worst, [stopped.get(g.c) for g in groups if len(g.rows)], flags


def _line(label, worst, **figures):
    _say('%s %s | %s', label, ' '.join('%s=%s' % kv for kv in sorted(figures.items())),
         ' '.join('%s %.3g' % (k, v[0]) for k, v in sorted(worst.items())))


def _leg(gpu_device, name, leg):
    cs = P.case(name)
    _, pp, tp, use_lnl, stops = P.LEG[leg]
    eps = P.leg_eps(name, leg)
    worst, st, flags = _run(gpu_device, cs, (pp, tp), use_lnl, eps, (name, leg))
    if stops:
        assert any(t is not None and t < cs.T for t in st) and any(t is None or t >= cs.T for t in st), (name, leg, 'stops', st)
        if cs.spread:
            assert any(t is not None and t < G.SP_LOOK for t in st) and G.SP_LOOK in st and any(t is not None and t > G.SP_LOOK for t in st), st
    else:
        assert st == [None] * len(st)
        for c in cs.gadget_groups:
            assert all(flags[c][k] > 0 for k in ('zero', 'gradual', 'left')), (name, c, 'the extreme states were not met', flags[c])
    _line(name, worst, leg=leg, eps='%.6g' % eps, steps=cs.T, groups=cs.n_groups, classes='/'.join(str(n) for n in cs.class_counts()),
          stops=','.join(str(t) for t in st),
          extreme=';'.join('g%d:%d/%d/%d' % (c, flags[c]['zero'], flags[c]['gradual'], flags[c]['left']) for c in cs.gadget_groups))


@pytest.mark.parametrize('leg', [l[0] for l in P.LEGS])
def test_one_workgroup_classes(gpu_device, leg):
    """a wave per cell, 256 threads, 512 threads with LDS tables, 512 threads with the global workspace: the cells on either side of
    Kc 256 / 1024 / 3840 and of 4096 entries, one of each class with the ladder gadget, and Kc 1, Kc 2, one row"""
    assert all(n > 0 for n in P.case('classes').class_counts()[:4])
    _leg(gpu_device, 'classes', leg)


@pytest.mark.parametrize('leg', [l[0] for l in P.LEGS])
def test_spread_class(gpu_device, leg):
    """every group spread: columns of 32 | 33, 64 m | 64 m + 1, 4096 | 4097, 256 m | 256 m + 1 entries (one lane | a wave | the
    workgroup), groups of exactly one chunk of 1024 rows, 1025 rows and one row, one group with the ladder gadget; T = 12 steps cross
    the host's look after 8 iterations"""
    cs = P.case('spread')
    assert cs.class_counts()[4] == cs.n_groups and all(n > 0 for n in cs.spread_tiers()) and cs.T > G.SP_LOOK + 1
    _leg(gpu_device, 'spread', leg)
    _say('spread tiers: columns by tier lane/wave/workgroup = %s', '/'.join(str(n) for n in cs.spread_tiers()))


@pytest.mark.parametrize('spread', [0, 1])
@pytest.mark.parametrize('key', P.DEGENERATE)
def test_degenerate_groups(gpu_device, key, spread):
    """one step each, in both classes: rows without entries, Kc = 0, Kc = K, K = 1 and 2, a group of unique rows only (theta = 0 / 0 at
    theta_prior = 0), an empty group"""
    cs = P.degenerate_case(key, spread)
    for priors in P.DEGENERATE_PRIORS:
        worst, st, _ = _run(gpu_device, cs, priors, False, 0.0, (key, spread, priors))
        _line('degenerate', worst, case=key, spread=spread, priors='%s/%s' % priors, classes='/'.join(str(n) for n in cs.class_counts()))
