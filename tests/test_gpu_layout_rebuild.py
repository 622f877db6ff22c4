"""`-m gpu`: tsem_build_layout on a handle that already has a layout (telescope_amd/csrc/tsem_setup.hip) — the two recovery paths
that run it a second time must leave what a fresh engine with the same options gets: tsem_prepare_likelihood against option
"use_likelihood" set before tsem_set_model, tsem_fallback_twopass (called on a healthy fused handle; nothing times out) against
option "em_kernel" = two-pass.  Equal means the fields of layout_info() and the (row slot << 16 | column slot) words of every
sub-block (block, part) through tsem_debug_subblock.  The matrix: 5 000 generated rows x 3 000 columns, ~40 entries per row, 5 %
unique rows.

Two fields of layout_info() are left out.  `fallbacks` counts the fall-backs themselves.  `max_subblock` describes the fused layout
and is written only by a build for the fused kernel: a handle that fell back still shows the largest sub-block of the fused layout
it had (3519 here), a fresh two-pass engine 0 (profiles/r17_layout_steps.txt); no kernel's launch reads it.

The words of the two-pass layout come from k_sb_fill, which orders a strand by its atomics (the words are compared sorted) and deals
the entries of a column that has several slots over them in that order too: two engines made alike then differ in the column halves
of that column's words.  With split columns (the default, `hot_cols` 1 here) the row halves are compared, and the same pair is made
once more with option "hot_split" = 0, where every sorted word must be equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EMK_TWOPASS = 1
NOT_COMPARED = ('fallbacks', 'max_subblock')      # see the module's text
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _engine(gpu_device, options=(), rebuild=None):
    """an _lib.Engine that remembers a HIP error (TSEM_ERR_HIP, TSEM_ERR_TIMEOUT) for the fixture above, with the matrix and the model"""
    from telescope_amd import _lib, synthetic
    from telescope_amd.likelihood import score_lut

    class Engine(_lib.Engine):
        def _ck(self, rc):
            if rc in (-2, -4):
                _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
            _lib.Engine._ck(self, rc)
    eng = Engine(gpu_device)
    for key, v in options:
        eng.set_option(key, v)
    eng.generate(0, 5000, 3000, synthetic.poisson_cdf_u32(40), 42, 1, 0.05)
    eng.set_lut(score_lut(eng.max_score()))
    stats, pisum0, cnt, hsh = eng.rowstats()
    eng.set_model(stats, pisum0, cnt, hsh, 0.0, 200000.0)
    if rebuild:
        getattr(eng, rebuild)()
    return eng


def _info_diff(a, b):
    ia, ib = a.layout_info(), b.layout_info()
    return {k: (ia[k], ib[k]) for k in ia if k not in NOT_COMPARED and ia[k] != ib[k]}, len(ia) - len(NOT_COMPARED)


def _same_words(a, b, label):
    """the sub-blocks of two engines word for word; returns how many were compared"""
    ia, ib = a.layout_info(), b.layout_info()
    assert (ia['nb'], ia['P'], ia['row_order'], ia['hot_cols']) == (ib['nb'], ib['P'], ib['row_order'], ib['hot_cols']), (label, ia, ib)
    cap = int(ia['nnz_pad']) + 64                                      # (no sub-block is longer than all of them together)
    for blk in range(int(ia['nb'])):
        for part in range(int(ia['P'])):
            wa, wb = a.debug_subblock(blk, part, cap=cap), b.debug_subblock(blk, part, cap=cap)
            assert len(wa) < cap and len(wa) == len(wb), (label, 'sub-block', blk, part, len(wa), len(wb))
            if not ia['row_order']:                                    # k_sb_fill: see the module's text
                wa, wb = (np.sort(wa >> 16), np.sort(wb >> 16)) if ia['hot_cols'] else (np.sort(wa), np.sort(wb))
            assert np.array_equal(wa, wb), (label, 'sub-block', blk, part, len(wa), np.flatnonzero(wa != wb)[:5])
    return int(ia['nb'] * ia['P'])


def test_prepare_likelihood_gives_the_layout_of_the_option(gpu_device):
    a = _engine(gpu_device, (('use_likelihood', 1),))
    b = _engine(gpu_device, (), 'prepare_likelihood')
    ia = a.layout_info()
    assert ia['lnl_fused'] == 1 and ia['fused'] == 1 and ia['row_order'] == 1, ia
    diff, n = _info_diff(a, b)
    print('LAYOUT prepare_likelihood: %d fields compared, %d differ %r; %d sub-blocks equal as stored' % (n, len(diff), diff, _same_words(a, b, 'prepare_likelihood')))
    assert not diff, ('layout_info differs (fresh, rebuilt)', diff)
    a.close()
    b.close()


def _fallback_pair(gpu_device, hot_split):
    a = _engine(gpu_device, (('em_kernel', EMK_TWOPASS), ('hot_split', hot_split)))
    b = _engine(gpu_device, (('hot_split', hot_split),), 'fallback_twopass')
    ia, ib = a.layout_info(), b.layout_info()
    assert ia['fused'] == 0 and ib['fused'] == 0 and ib['fallbacks'] == 1 and (ia['hot_cols'] > 0) == (hot_split == 1), (ia, ib)
    return a, b


@pytest.mark.parametrize('hot_split', (1, 0))
def test_fallback_gives_the_sub_blocks_of_the_two_pass_option(gpu_device, hot_split):
    a, b = _fallback_pair(gpu_device, hot_split)
    n = _same_words(a, b, 'fallback_twopass')
    print('LAYOUT fallback_twopass, hot_split %d: %d sub-blocks equal (%s, sorted)' % (hot_split, n, 'row halves' if hot_split else 'words'))
    a.close()
    b.close()


def test_fallback_gives_the_layout_info_of_the_two_pass_option(gpu_device):
    a, b = _fallback_pair(gpu_device, 1)
    diff, n = _info_diff(a, b)
    print('LAYOUT fallback_twopass: %d fields compared, %d differ (fresh, rebuilt) %r' % (n, len(diff), diff))
    a.close()
    b.close()
    assert not diff, ('layout_info differs (fresh, rebuilt)', diff)
