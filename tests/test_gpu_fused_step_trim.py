"""`-m gpu`: ONE tsem_em_pass of the fused kernel against the exact reference of tests/_em_pass_reference.py (exact_colsums,
colsum_bound: the bound formula of tests/test_gpu_em_pass_exact.py, parameters from parameter_set), at the shapes where the data
waves' step can go wrong: the row sums (fz_row_sums: at most two atomics per lane, the rest behind a wave-uniform branch), the
profiling instantiation (k_em_fused<..., PROF = true>, option "fused_prof") next to the product kernels, and the hand-off recovery.

  row lengths      per part 1, 2, 3, 4, 5, 7, 8, 9, runs of 130 - 300 entries in one part (more than two lanes: the shift loop iterates),
                   row slots that a part leaves empty — read back from the layout's own sub-blocks (tsem_debug_subblock), asserted
  sub-block tails  last quads with 1, 2, 3 real entries (asserted from the sub-blocks); wholly idle tail waves (geometry 2 / 3 on
                   rows of 2 - 6 entries, whose sub-blocks fill half a register tile)
  pipeline depth   teams that walk 0, 1, 2, 5, 6, 7 blocks — fewer than the ring of six register sets is deep, and just past it —
                   read from the start-up stamps of the profiled launch: what every team really got
  instantiations   teams of 1 and 4, fp64 entries and score codes (value_format 1 / 2), geometry 0, 2, 3; sorted_fill 0 (one atomic per
                   entry: no row sums in registers)
Every case prints a `STEPTRIM` line with the figure it asserts on (`pytest -s`)."""
import numpy as np
import pytest

import _em_pass_reference as E

pytestmark = pytest.mark.gpu
PRIORS = (0, 200000)
PSET = 'decades'
_refs, _mats = {}, {}
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


def _say(fmt, *a):
    print('STEPTRIM ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _matrix(mkey):
    """row_shape / row_shape_p1 / short / ('ring', rows) of _em_pass_reference, and 'short_p1': rows of 2 - 6 entries over 4000
    columns (one column part holds at most 7680)"""
    if mkey not in _mats:
        if mkey == 'short_p1':
            _mats[mkey] = E.short_row_matrix(3000, 4000)
        elif isinstance(mkey, tuple):
            _mats[mkey] = E.matrix(*mkey)
        else:
            _mats[mkey] = E.matrix(mkey, E.REDUCED.get(mkey))
    return _mats[mkey]


def _ref(mkey):
    """the shared exact reference of a matrix under PSET, computed once and left unchanged"""
    if mkey not in _refs:
        raw = _matrix(mkey)
        pi, theta = E.parameter_set(PSET, raw)
        _refs[mkey] = E.PassReference(raw, E.lut(raw), pi, theta, want_lnl=False)
        assert _refs[mkey].fair == [], (mkey, _refs[mkey].fair)
    return _refs[mkey]


class Model(object):
    """an engine holding the matrix `mkey`, its model set through the C ABI, the parameters of the shared reference"""

    def __init__(self, gpu_device, mkey, options):
        from telescope_amd import _lib

        class Engine(_lib.Engine):
            def _ck(self, rc):
                if rc in (_lib.ERR_HIP,):
                    _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
                _lib.Engine._ck(self, rc)
        self.raw, self.ref, self.K = _matrix(mkey), _ref(mkey), _matrix(mkey).shape[1]
        self.eng = eng = Engine(gpu_device)
        for key, v in options:
            eng.set_option(key, v)
        raw = self.raw
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), self.K, E.lut(raw))
        eng.max_score()
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, *PRIORS)
        self.info = eng.layout_info()
        o = dict(options)
        assert self.info['fused'] == 1 and self.info['split'] == 0 and self.info['nb'] > 0, (options, self.info)
        assert self.info['P'] == o['parts'], (options, self.info)
        assert self.info['value_bytes'] == (2 if o['value_format'] == 2 else 8), (options, self.info)
        assert self.info['index_bytes'] == (4 if o['value_format'] == 2 else 3), (options, self.info)
        if 'geometry' in o:
            assert self.info['geometry'] == o['geometry'], (options, self.info)
        if 'block_rows' in o:
            assert self.info['R'] == o['block_rows'], (options, self.info)
        assert self.info['row_order'] == (0 if o.get('sorted_fill') == 0 else 1), (options, self.info)
        eng.set_params(self.ref.pi, self.ref.theta)

    def pass_fraction(self, label, path=E.FUSED):
        """one tsem_em_pass; the largest |red_j - exact_j| as a fraction of its bound, asserted <= 1; exact zeros exactly 0"""
        ref, P = self.ref, (int(self.info['P']) if path == E.FUSED else 0)
        self.eng.em_pass()
        red = self.eng.read_reduce(0, self.K + 2)
        assert not np.any(np.isnan(red)), (label, 'NaN in the reduce buffer')
        assert red[self.K] == 0.0 and red[self.K + 1] == 0.0, (label, 'time-out word / carried value', red[self.K:])
        frac, j = E.colsum_fraction(red[:self.K], ref.sums, ref.cnt, ref.lenmax, ref.gradual, path, P)
        zero = (ref.sums == 0) & (ref.gradual == 0)
        bad = np.flatnonzero(zero & (red[:self.K] != 0))
        _say('%s: column sums %.3f of the bound (column %d, %d entries, longest row %d)', label, frac, j, ref.cnt[j], ref.lenmax[j])
        assert len(bad) == 0, (label, 'columns that are exactly 0', bad[:5], red[bad[:5]])
        assert frac <= 1.0, (label, 'column', j, float(red[j]), float(ref.sums[j]), frac)
        return frac


def _name(options):
    return '-'.join('%s%d' % (k, v) for k, v in options)


def _sub_block_shapes(m):
    """What the layout's sub-blocks hold, from their own index words (row slot << 16 | column slot, in stored order): the lengths of
    the runs of equal rows, whether some row slot of a block is missing from a part, and the real entries of the last quads.  A
    sub-block is padded to whole waves with its last row and column slot 0 (value 0)."""
    info = m.info
    runs, tails, gaps, n_real = set(), set(), 0, 0
    for blk in range(info['nb']):
        slots = []
        for part in range(info['P']):
            w = m.eng.debug_subblock(blk, part, cap=8192).astype(np.int64)
            if len(w) == 0:
                slots.append(np.zeros(0, dtype=np.int64))
                continue
            rows = w >> 16
            pad_word = rows[-1] << 16
            pad = 0
            while pad < len(w) - 1 and w[len(w) - 1 - pad] == pad_word and rows[len(w) - 2 - pad] == rows[-1]:
                pad += 1                                      # (a real entry of column slot 0 comes first in its row: at most one short)
            real = len(w) - pad
            n_real += real
            tails.add(real % 4)
            edges = np.flatnonzero(np.diff(rows[:real]) != 0)
            runs.update(np.diff(np.concatenate([[-1], edges, [real - 1]])).tolist())
            slots.append(np.unique(rows[:real]))
        allrows = np.unique(np.concatenate(slots))
        gaps += sum(len(allrows) - len(s) for s in slots)
    return runs, tails, gaps, n_real


SHAPE_CASES = [('row_shape', 4, f, g) for f in (1, 2) for g in (0, 2, 3)] + [('row_shape_p1', 1, f, 0) for f in (1, 2)] + \
              [('short', 4, f, g) for f in (1, 2) for g in (2, 3)] + [('short_p1', 1, f, g) for f in (1, 2) for g in (2, 3)]


@pytest.mark.parametrize('mkey,parts,fmt,geo', SHAPE_CASES, ids=lambda v: str(v))
def test_one_pass_on_every_instantiation(gpu_device, mkey, parts, fmt, geo):
    """teams of 1 and 4 x both entry formats x geometry 0, 2, 3 in row order: the row-shape matrix (rows of 2 ... 1000 entries and one
    of K - 2) and rows of 2 - 6 entries, whose sub-blocks leave the tail waves of a step wholly idle"""
    options = (('parts', parts), ('value_format', fmt), ('geometry', geo))
    m = Model(gpu_device, mkey, options)
    m.pass_fraction('%s %s' % (mkey, _name(options)))
    info = m.eng.layout_info()
    assert info['fallbacks'] == 0, info
    if mkey == 'short':                                      # 768 / 1152 row slots x ~4 entries over 4 parts: a third of the tile of 3328
        assert 0 < info['max_subblock'] <= 3328 - 256, ('no wave of the register tile is left idle', info)


@pytest.mark.parametrize('mkey,parts', [('row_shape', 4), ('row_shape_p1', 1)])
def test_the_row_shapes_reach_the_sub_blocks(gpu_device, mkey, parts):
    """what the cases above rely on, read from the layout: per part, runs of 1 (teams of 4), 2, 3, 4, 5, 7, 8, 9 and of 130 - 300
    entries, row slots without an entry in some part (teams of 4), last quads with 1, 2 and 3 real entries"""
    options = (('parts', parts), ('value_format', 1), ('geometry', 0), ('block_rows', 64))
    m = Model(gpu_device, mkey, options)
    runs, tails, gaps, n_real = _sub_block_shapes(m)
    _say('%s %s: %d sub-blocks, run lengths %s ... longest %d, %d empty (row slot, part) pairs, real entries of the last quads mod 4 %s, '
         '%d real entries (nnz_amb %d)', mkey, _name(options), m.info['nb'] * parts, sorted(runs)[:12], max(runs), gaps, sorted(tails), n_real,
         m.info['nnz_amb'])
    want = {2, 3, 4, 5, 7, 8, 9} | ({1} if parts > 1 else set())
    assert want <= runs, ('run lengths missing from the sub-blocks', sorted(want - runs))
    assert any(130 <= r <= 300 for r in runs), ('no run spans 33 - 75 lanes', sorted(runs)[-10:])
    assert {1, 2, 3} <= tails, ('last quads', sorted(tails))
    if parts > 1:
        assert gaps > 0, 'every row has entries in every part'
    m.pass_fraction('%s %s' % (mkey, _name(options)))


@pytest.mark.parametrize('fmt', [1, 2])
def test_strand_order_keeps_one_atomic_per_entry(gpu_device, fmt):
    """sorted_fill 0: the strand-transposed layout, where neighbouring entries never share a row and every entry has its own atomic"""
    options = (('parts', 4), ('value_format', fmt), ('sorted_fill', 0))
    m = Model(gpu_device, 'row_shape', options)
    m.pass_fraction('row_shape %s' % _name(options))


def _team_blocks(eng):
    """blocks per team of the last profiled launch, from the start-up stamps of the workgroups whose team formed"""
    t = eng.fused_startup().astype(np.int64)
    t = t[t[:, 4] > 0]
    team, nblk = (t[:, 7] >> 32) & 0xFFFF, t[:, 7] & 0xFFFF
    per_team = {}
    for a, b in zip(team.tolist(), nblk.tolist()):
        assert per_team.setdefault(a, b) == b, 'members of one team disagree about their blocks'
    return per_team


@pytest.mark.parametrize('parts,fmt,fill', [(p, f, x) for p, f in ((1, 1), (4, 2), (4, 1)) for x in (0.5, 1.5, 5.5, 6.5)])
def test_fewer_blocks_than_the_pipeline_is_deep(gpu_device, parts, fmt, fill):
    """blocks of 64 rows, `fill` blocks per team on average: teams walk floor(fill) and ceil(fill) blocks — 0 / 1, 1 / 2, 5 / 6, 6 / 7
    against six register sets, a prefetch distance of 2 and a scatter lag of 4 — read from the profiled launch itself"""
    import torch
    teams = max(1, int(torch.cuda.get_device_properties(gpu_device).multi_processor_count) // parts)
    rows = int(fill * teams * 64 / 0.94)
    mkey = ('ring', rows)
    options = (('parts', parts), ('value_format', fmt), ('block_rows', 64))
    m = Model(gpu_device, mkey, options)
    m.eng.set_option('fused_prof', 2)                        # the start-up stamps only
    m.pass_fraction('ring %d rows %s' % (rows, _name(options)))
    got = _team_blocks(m.eng)
    depths = set(got.values())
    nb, T = m.info['nb'], len(got)
    _say('ring %d rows %s: %d blocks over %d teams that formed: blocks per team %s', rows, _name(options), nb, T, sorted(depths))
    assert sum(got.values()) == nb, ('the teams walk every block once', sum(got.values()), nb)
    assert {int(np.floor(fill)), int(np.ceil(fill))} <= depths, ('teams with these block counts were wanted', fill, sorted(depths), nb, T)


@pytest.mark.parametrize('parts,fmt', [(1, 1), (1, 2), (4, 1), (4, 2)])
def test_profiled_pass_gives_the_same_sums_and_a_timeline(gpu_device, parts, fmt):
    """option fused_prof = 1: the pass runs the timeline instantiation — the same sums within the bound, before and after the option is
    set, and for the first steps of team 0 / member 0 non-zero stamps that increase from step to step"""
    mkey = 'row_shape' if parts > 1 else 'row_shape_p1'
    options = (('parts', parts), ('value_format', fmt))
    m = Model(gpu_device, mkey, options)
    m.pass_fraction('%s %s product kernel' % (mkey, _name(options)))
    m.eng.set_option('fused_prof', 1)
    m.pass_fraction('%s %s timeline kernel' % (mkey, _name(options)))
    t = m.eng.fused_prof().astype(np.int64)
    blocks = _team_blocks(m.eng)
    steps = min(blocks[0] + 5, 8)                            # team 0 runs its blocks + 5 steps
    start, barrier = t[:steps, 0], t[:steps, 4]
    _say('%s %s: team 0 walks %d blocks; clocks per step %s', mkey, _name(options), blocks[0], np.diff(start).tolist())
    assert blocks[0] >= 1 and steps >= 6, blocks
    assert np.all(t[:steps, [0, 1, 2, 3, 4]] > 0), ('data wave 0', t[:steps, :5])
    assert np.all(t[:steps, [5, 6, 7, 10]] > 0), ('exchange wave 0', t[:steps, 5:11])
    assert np.all(barrier > start) and np.all(start[1:] >= barrier[:-1]), (start, barrier)


def test_no_timeline_kernel_for_teams_of_five(gpu_device):
    """the timeline instantiation exists for teams of 1 - 4: elsewhere the profiled pass fails with a text, it does not run unprofiled"""
    from telescope_amd import _lib
    m = Model(gpu_device, 'row_shape', (('parts', 5), ('value_format', 1)))
    m.eng.set_option('fused_prof', 1)
    with pytest.raises(_lib.EngineError) as ei:
        m.eng.em_pass()
    assert ei.value.code == _lib.ERR_ARG and 'fused_prof' in str(ei.value), str(ei.value)


def test_hand_off_time_out_recovers_end_to_end(gpu_device):
    """fused_dbg = 32: the pass behaves like a hand-off time-out; the update refuses to commit, tsem_recover_timeout rebuilds the
    layout for the two-pass kernels, and the redone pass gives the sums within the bound of that path"""
    from telescope_amd import _lib
    m = Model(gpu_device, 'row_shape', (('parts', 4), ('value_format', 1), ('fused_dbg', 32)))
    m.eng.em_pass()
    with pytest.raises(_lib.EngineError) as ei:
        m.eng.em_update()
    assert ei.value.code == _lib.ERR_TIMEOUT
    pi, theta = m.eng.get_params(_lib.Z_CUR)
    assert np.array_equal(pi, m.ref.pi) and np.array_equal(theta, m.ref.theta), 'the refused update touched the parameters'
    assert m.eng.recover_timeout() is True
    m.info = m.eng.layout_info()
    assert m.info['fused'] == 0 and m.info['fallbacks'] == 1, m.info
    m.pass_fraction('row_shape after the recovery', path=E.UNTAGGED)
