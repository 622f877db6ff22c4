"""CPU (`-m "not gpu"`): ties tests/_report_reference.py down before tests/test_gpu_report_instances.py holds the streaming report
kernels against it.

* the reference's sums equal `OracleModel.reassign(...).sum(0)` (within the limit for `conf` and `average`, exactly for the
  integer-valued methods) on every input, both sources of z, every conf_prob of the GPU legs;
* every class matrix selects its class under the 0.5 % rule of report_capacity, has skewed columns and more columns in use than the
  LDS of k_report_rows holds popularity ids;
* by the reference alone every leg holds at least 20 single winners, two-way ties, wider ties, rows with an empty pattern and rows
  passing `conf`, and at conf_prob 0.45 at least 20 rows where several entries pass;
* at most 1 % of the rows are unclear (their expected entries are the oracle's) in any leg, none at 0.9 and 0.45 for the final z
  with scores up to 400.  Rows of one stored entry are not counted: their exact z = 1 sits on conf_prob = 1.0 by construction, and
  their fp64 z is the same two operations on every side (the reference takes the oracle's entries there at every conf_prob).

Each test prints the figures it asserts on (`pytest -s`)."""
import time

import numpy as np
import pytest

import _report_reference as P
import _rowpass_reference as R

THRESHOLDS = {R.INITIAL: (0.9,), R.CUR: (0.9, 0.45, 0.5, 1.0)}
INTEGER_METHODS = ('exclude', 'choose', 'unique', 'all')
CASES = [(c, s) for c in P.CLASSES for s in P.SCORES] + [('cold', 400)]


@pytest.mark.parametrize('c', P.CLASSES)
def test_each_class_matrix_selects_its_class(c):
    for s in P.SCORES:
        raw = P.class_case(c, s)[0]
        lens = np.diff(raw.indptr)
        assert raw.shape == (P.N_ROWS, P.K) and P.capacity_class(lens) == c, (c, s, P.capacity_class(lens))
        assert lens[0] == c and lens[-1] == c - 1
        assert set(lens) >= {0, 1, 2, c // 2, c // 2 + 1, c - 1, c, c + 1, 2 * c, 4 * c, 257, 513, 700, 1025}
        assert np.count_nonzero(lens > c) == 8                           # 0.27 % of the rows
        # skewed columns, and yet more of them in use — by rows the streaming kernels serve themselves — than k_report_rows' LDS holds
        # ids: (160 KiB - 2 KiB - the score table - 16 B x Hs) / 8 B is below 15 400 with any table (tsem_report.hip, report_streaming)
        count = np.sort(np.bincount(raw.indices, minlength=P.K))[::-1]
        inside, outside = P.ids_beside(raw, 15400, 3, 16, c)
        print('class %d, scores to %d: %d entries on %d columns, the 200 most popular hold %d; beside 15 400 ids: %s inside, %s outside'
              % (c, s, raw.nnz, np.count_nonzero(count), count[:200].sum(), inside, outside))
        assert count[:200].sum() >= 5 * 200 * raw.nnz / P.K, (c, s, count[:200].sum(), raw.nnz)
        assert outside[0] >= 1000 and inside[0] >= 1000, (c, s, inside, outside)


def test_cold_matrix_holds_every_scan_step():
    raw, lut, pi, theta = P.cold_case()
    lens = set(np.diff(raw.indptr))
    for e in (8, 16):
        for g in P.SCAN_STEPS:
            assert lens >= set(range((g - 1) * e + 1, g * e + 1)), (e, g)
    assert raw.shape[1] == P.K_COLD and len(np.unique(raw.indices)) > 44000      # more columns in use than any LDS table holds


@pytest.mark.parametrize('which', [R.INITIAL, R.CUR])
@pytest.mark.parametrize('c,max_score', CASES)
def test_reference_sums_equal_the_oracles(c, max_score, which):
    t0 = time.time()
    ref = P.reference(c, max_score, which)
    raw = ref.raw
    n = raw.shape[0]
    group = P.group_map(n)
    for thresh in THRESHOLDS[which]:
        for m in R.METHODS if thresh == 0.9 else P.REPORT_METHODS:
            o = R.oracle_assigned(ref.ref.om, raw, m, thresh, which, ref.picks)
            want = np.bincount(raw.indices, weights=o, minlength=raw.shape[1])
            s, lim = ref.sums(m, thresh)
            if m in INTEGER_METHODS:
                assert np.array_equal(s.astype(np.float64), want), (c, max_score, which, thresh, m)
            else:
                frac = P.fraction(want, s, lim)
                print('reference %s/%s/%s %s at %.2f: the oracle lies at %.3f of the limit' % (c, max_score, which, m, thresh, frac))
                assert frac <= 1.0, (c, max_score, which, thresh, m)
        rows, counts = ref.ties(thresh)
        nbo = ref.ref.nbo
        assert np.array_equal(rows, np.flatnonzero(nbo > 1)) and np.array_equal(counts, nbo[nbo > 1]), (c, max_score, which, thresh)
    gs, _ = ref.group_sums('exclude', 0.9, group, P.GROUPS)
    in_groups, _ = ref.sums('exclude', 0.9, group >= 0)
    assert np.array_equal(gs.sum(0), in_groups) and np.any(group < 0) and set(group) == set(range(-1, P.GROUPS))
    print('reference %s/%s/%s: %.2f s' % (c, max_score, which, time.time() - t0))


@pytest.mark.parametrize('which', [R.INITIAL, R.CUR])
@pytest.mark.parametrize('c,max_score', CASES)
def test_every_leg_holds_every_kind_of_row(c, max_score, which):
    ref = P.reference(c, max_score, which)
    n = ref.raw.shape[0]
    for thresh in THRESHOLDS[which] if c != 'cold' else (0.9,):          # (the COLD matrix runs at 0.9 only)
        k = ref.census(thresh)
        print('census %s/%s/%s at %.2f: %s' % (c, max_score, which, thresh, k))
        for kind in ('single', 'two_way', 'wider', 'empty', 'conf'):
            assert k[kind] >= 20, (c, max_score, which, thresh, kind, k)
        if thresh == 0.45:
            assert k['conf_several'] >= 20, (c, max_score, thresh, k)
        assert k['unclear'] <= 0.01 * n, (c, max_score, which, thresh, k)
        # the rows left out of that cap sit ON conf_prob 1.0: none at a lower conf_prob, and never more than the rows whose largest exact z
        # is within 2 bound(len) of 1 (every row of one entry is one), so that they cannot grow unnoticed
        assert k['on_one'] <= (k['near_one'] if thresh >= 1.0 else 0), (c, max_score, which, thresh, 'rows left out of the cap', k['on_one'],
                                                                        'rows with the largest z at 1', k['near_one'], k)
        if which == R.CUR and max_score == 400 and thresh in (0.9, 0.45):
            assert k['unclear'] == 0, (c, max_score, thresh, k)
