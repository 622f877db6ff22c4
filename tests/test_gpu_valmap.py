"""`-m gpu`: the value map of the layouts the fused kernel reads (telescope_amd/csrc/tsem_valmap.h: a sub-block's fp64 values grouped by
wave, so that each of a lane's two 16-byte loads takes whole 128-byte lines).

  read-back   every sub-block's values in entry order (tsem_debug_subblock_values) are lut[raw] of the CSR entries its index words
              (tsem_debug_subblock) name — all three writers of the values (row-order fill, its padding, strand-transposed fill), the
              3-byte and the 4-byte index (split layout) — at block_rows = 64, where the sub-blocks have 16, 32, 48 and 0 quads modulo
              the group of 64, and some fewer than one group: asserted;
  one pass    ONE tsem_em_pass and ONE tsem_lnl_pass against the exact reference of tests/_em_pass_reference.py with the bound
              formula of tests/test_gpu_em_pass_exact.py, fp64 entries: teams of 1 and 4, geometry 0 / 2 / 3, sorted_fill 0 and 1, a
              split layout, and the two-pass kernels on the layout tsem_recover_timeout rebuilds (values entry by entry again).
Every case prints a `VALMAP` line with the figures it asserts on (`pytest -s`)."""
import numpy as np
import pytest

import _em_pass_reference as E

pytestmark = pytest.mark.gpu
LD = E.LD
PRIORS = (0, 200000)
PSET = 'decades'
_refs, _mats = {}, {}
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


def _say(fmt, *a):
    print('VALMAP ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _matrix(mkey):
    if mkey not in _mats:
        _mats[mkey] = E.matrix(*mkey) if isinstance(mkey, tuple) else E.matrix(mkey, E.REDUCED.get(mkey))
    return _mats[mkey]


def _ref(mkey):
    """the shared exact reference of a matrix under PSET (previous = current), computed once and left unchanged"""
    if mkey not in _refs:
        raw = _matrix(mkey)
        pi, theta = E.parameter_set(PSET, raw)
        _refs[mkey] = E.PassReference(raw, E.lut(raw), pi, theta)
        assert _refs[mkey].fair == [], (mkey, _refs[mkey].fair)
    return _refs[mkey]


def _name(options):
    return '-'.join('%s%d' % (k, v) for k, v in options)


class Model(object):
    """an engine holding the matrix `mkey` as fp64 entries, its model set through the C ABI"""

    def __init__(self, gpu_device, mkey, options):
        from telescope_amd import _lib

        class Engine(_lib.Engine):
            def _ck(self, rc):
                if rc in (_lib.ERR_HIP,):
                    _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
                _lib.Engine._ck(self, rc)
        self.raw, self.K = _matrix(mkey), _matrix(mkey).shape[1]
        self.lut = E.lut(self.raw)
        self.eng = eng = Engine(gpu_device)
        for key, v in options:
            eng.set_option(key, v)
        raw = self.raw
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), self.K, self.lut)
        eng.max_score()
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, *PRIORS)
        self.info = info = eng.layout_info()
        o = dict(options)
        assert info['fused'] == 1 and info['nb'] > 0 and info['value_bytes'] == 8, (options, info)
        assert info['split'] == o.get('split', 0), (options, info)
        assert info['index_bytes'] == (4 if info['split'] else 3), (options, info)
        assert info['P'] == o['parts'], (options, info)
        if 'geometry' in o:
            assert info['geometry'] == o['geometry'], (options, info)
        if 'block_rows' in o:
            assert info['R'] == o['block_rows'], (options, info)
        assert info['row_order'] == (0 if o.get('sorted_fill') == 0 else 1), (options, info)

    def path(self):
        i = self.info
        if i['split'] == 1:
            return E.SPLIT, 0
        if i['fused'] == 1:
            return E.FUSED, int(i['P'])
        return E.UNTAGGED, 0

    def one_pass_each(self, ref, label):
        """one tsem_lnl_pass (previous = current) and one tsem_em_pass; both figures printed, then asserted <= 1"""
        path, P = self.path()
        self.eng.set_params(ref.pi, ref.theta)
        self.eng.set_params(ref.pi, ref.theta)
        self.eng.lnl_pass()
        lnl = float(self.eng.read_reduce(self.K, 1)[0])
        lfrac = float(abs(LD(lnl) - ref.lnl) / ref.lnl_limit_P(P)) if np.isfinite(lnl) else np.inf
        self.eng.em_pass()
        red = self.eng.read_reduce(0, self.K + 2)
        assert not np.any(np.isnan(red)), (label, 'NaN in the reduce buffer')
        assert red[self.K] == 0.0 and red[self.K + 1] == 0.0, (label, 'time-out word / carried value', red[self.K:])
        frac, j = E.colsum_fraction(red[:self.K], ref.sums, ref.cnt, ref.lenmax, ref.gradual, path, P)
        zero = (ref.sums == 0) & (ref.gradual == 0)
        bad = np.flatnonzero(zero & (red[:self.K] != 0))
        _say('%s: column sums %.3f of the bound (column %d, %d entries, longest row %d); lnl %.3g of its limit', label, frac, j, ref.cnt[j],
             ref.lenmax[j], lfrac)
        assert len(bad) == 0, (label, 'columns that are exactly 0', bad[:5], red[bad[:5]])
        assert frac <= 1.0, (label, 'column', j, float(red[j]), float(ref.sums[j]), frac)
        assert lfrac <= 1.0, (label, 'lnl', lnl, float(ref.lnl), lfrac)


# ---- the read-back --------------------------------------------------------------------------------------------------------------------
READBACK = [('ring', (('parts', 1), ('value_format', 1), ('block_rows', 64))),
            ('row_shape', (('parts', 4), ('value_format', 1), ('block_rows', 64))),
            ('row_shape', (('parts', 4), ('value_format', 1), ('block_rows', 64), ('sorted_fill', 0))),
            ('row_shape', (('split', 1), ('parts', 5), ('value_format', 1), ('block_rows', 64)))]


def _read_back(m, label):
    """every sub-block: values in entry order against lut[raw] of the CSR entries the index words name; returns the quad counts"""
    raw, info = m.raw, m.info
    key_all = raw.indices.astype(np.int64) + np.repeat(np.arange(raw.shape[0], dtype=np.int64), np.diff(raw.indptr)) * m.K
    assert np.all(np.diff(key_all) > 0)                          # (CSR with sorted indices: the keys ascend)
    want_all = m.lut[raw.data]
    seen, nqs = [], []
    cap = int(info['nnz_pad']) + 64                              # (more than any sub-block holds)
    for blk in range(info['nb']):
        for part in range(info['P']):
            w = m.eng.debug_subblock(blk, part, cap=cap)
            v, rows, cols = m.eng.debug_subblock_values(blk, part, cap=cap)
            assert len(v) == len(w) and len(w) % 64 == 0 and len(w) < cap, (label, blk, part, len(v), len(w))
            nqs.append(len(w) // 4)
            real = v != 0.0
            assert np.all(rows[real] >= 0) and np.all(cols[real] >= 0), (label, blk, part)
            key = rows[real].astype(np.int64) * m.K + cols[real]
            at = np.searchsorted(key_all, key)
            assert np.all(at < len(key_all)) and np.array_equal(key_all[np.minimum(at, len(key_all) - 1)], key), \
                (label, blk, part, 'an index word names a cell the matrix does not store')
            assert np.array_equal(v[real].view(np.uint64), want_all[at].view(np.uint64)), (label, blk, part, 'values out of place')
            if info['row_order'] == 1 and (~real).any():          # the padding: behind the real entries, the last row and column slot 0 again
                first_pad = int(np.flatnonzero(~real)[0])
                assert not real[first_pad:].any() and np.all(w[first_pad:] == (w[first_pad] >> 16) << 16), (label, blk, part)
            seen.append(key)
    seen = np.concatenate(seen)
    assert len(seen) == info['nnz_amb'] and len(np.unique(seen)) == len(seen), (label, 'every stored entry of an ambiguous row once', len(seen), info['nnz_amb'])
    return np.array(nqs)


def test_values_read_back_in_entry_order(gpu_device):
    residues, short, whole = set(), 0, 0
    for mkey, options in READBACK:
        m = Model(gpu_device, mkey, options)
        nqs = _read_back(m, '%s %s' % (mkey, _name(options)))
        nz = nqs[nqs > 0]
        residues |= set((nz % 64).tolist())
        short += int((nz < 64).sum())
        whole += int((nz > 64).sum())
        _say('%s %s: %d sub-blocks, quads %d .. %d, quads mod 64: %s, %d shorter than a group', mkey, _name(options), len(nqs), nqs.min(), nqs.max(),
             dict(zip(*[x.tolist() for x in np.unique(nz % 64, return_counts=True)])), int((nz < 64).sum()))
        assert m.eng.layout_info()['fallbacks'] == 0
    assert residues == {0, 16, 32, 48}, residues
    assert short > 0 and whole > 0, (short, whole)


# ---- one pass against the exact reference ---------------------------------------------------------------------------------------------
def _o(parts, **kw):
    return (('parts', parts), ('value_format', 1)) + tuple(kw.items())


RING = ('ring', 40000)
PASS_CASES = [('row_shape', _o(4, geometry=0)), ('row_shape', _o(4, geometry=2)), ('row_shape', _o(4, geometry=3)),
              ('row_shape', _o(4, sorted_fill=0)), ('row_shape', (('split', 1),) + _o(5)),
              ('row_shape_p1', _o(1, geometry=0)),
              ('short', _o(4, geometry=2)), ('short', _o(4, geometry=3)), ('short', _o(4, sorted_fill=0)),
              (RING, _o(1, block_rows=64)), (RING, _o(4, block_rows=64)), (RING, _o(4, block_rows=64, sorted_fill=0))]


@pytest.mark.parametrize('mkey,options', PASS_CASES, ids=lambda v: _name(v) if isinstance(v, tuple) and isinstance(v[0], tuple) else str(v))
def test_one_em_pass_and_one_lnl_pass(gpu_device, mkey, options):
    m = Model(gpu_device, mkey, options)
    m.one_pass_each(_ref(mkey), '%s %s' % (mkey, _name(options)))
    info = m.eng.layout_info()
    assert info['fallbacks'] == 0 and info['fused'] == 1, info


def test_two_pass_kernels_on_the_rebuilt_layout(gpu_device):
    """fused_dbg = 32: the pass behaves like a hand-off time-out; tsem_recover_timeout rebuilds the layout for the two-pass kernels,
    which read the values entry by entry: the rebuilt layout is linear again, read back and run"""
    from telescope_amd import _lib
    m = Model(gpu_device, 'row_shape', _o(4) + (('fused_dbg', 32),))
    ref = _ref('row_shape')
    m.eng.set_params(ref.pi, ref.theta)
    m.eng.em_pass()
    with pytest.raises(_lib.EngineError) as ei:
        m.eng.em_update()
    assert ei.value.code == _lib.ERR_TIMEOUT
    assert m.eng.recover_timeout() is True
    m.info = m.eng.layout_info()
    assert m.info['fused'] == 0 and m.info['fallbacks'] == 1 and m.info['index_bytes'] == 4, m.info
    nqs = _read_back(m, 'row_shape rebuilt for the two-pass kernels')
    _say('rebuilt layout: %d sub-blocks, quads %d .. %d', len(nqs), nqs.min(), nqs.max())
    m.one_pass_each(ref, 'row_shape after the recovery')
