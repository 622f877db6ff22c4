"""`-m gpu`: the SUMMING outputs of the generic row pass (k_rowpass, telescope_amd/csrc/tsem_report.hip) on both sides of the 64-entry
boundary between its register tile and its sweeps.  tests/test_gpu_rowpass_entries.py pins what the pass hands out per stored entry at
every row length; this file pins, against the oracle, what it adds up or counts per row: best-hit counts and the tie list, the column
sums and masks of all six reassign methods (LDS hot slots; the split sums of option `reproducible`), the one-pass report, the sums over
a row list and the per-group sums — with `report_kernel` = 0, so that every one of them IS the generic pass.

One matrix: 602 rows x 700 columns, row lengths cycling through 1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513, scores from
three codes (exact ties of many widths in the initial z, on both sides of 64), three EM iterations of the engine, the parameters
downloaded and set again so that both sides hold the same numbers.  Integer-valued outputs are compared with array_equal, `conf` and
`average` with rtol 1e-12 / atol 1e-9 (the tolerances of test_packed_report_kernel_on_rows_of_every_shape between two orders of the same
additions)."""
import numpy as np
import pytest
import scipy.sparse as sp

import _rowpass_reference as R
from conftest import Opts

pytestmark = pytest.mark.gpu
LENGTHS = (1, 2, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513)
N, K, GROUPS = 43 * len(LENGTHS), 700, 7
THRESH = 0.9
FLOAT_METHODS = ('average', 'conf')


def _matrix():
    rng = np.random.RandomState(64)
    lens = np.tile(LENGTHS, N // len(LENGTHS))
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(K, l, replace=False)) for l in lens]).astype(np.int32)
    data = rng.randint(1, 4, indptr[-1]).astype(np.uint16)            # three distinct codes
    return sp.csr_matrix((data, indices, indptr), shape=(N, K))


def _same(got, want, method, what):
    if method in FLOAT_METHODS:
        assert np.allclose(got, want, rtol=1e-12, atol=1e-9), (what, method, float(np.max(np.abs(got - want))))
    else:
        assert np.array_equal(got, want), (what, method, np.flatnonzero(np.asarray(got) != np.asarray(want))[:5])


def _oracle(raw, pi, theta):
    """Per z (initial, final): best-hit counts, dense picks drawn as tests/test_gpu_round2.py draws them, and the six assignments on
    raw's stored entries — computed once, shared by both settings of `reproducible`."""
    from oracle.telescope_oracle import OracleModel
    om = OracleModel(raw, 0, 200000)
    out = {}
    for which in (R.INITIAL, R.CUR):
        R.numpy_z(om, raw, pi, theta, which)
        nb = R.oracle_best_counts(om, which)
        rows = np.flatnonzero(nb > 1)
        picks = np.zeros(N, np.int32)
        picks[rows] = np.random.default_rng(7).integers(0, 1 << 30, len(rows)) % nb[rows]
        out[which] = (nb, picks, {m: R.oracle_assigned(om, raw, m, THRESH, which, picks) for m in R.METHODS})
    return out


def test_summing_outputs_on_both_sides_of_the_tile_boundary(gpu_device):
    from telescope_amd import _lib
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    raw = _matrix()
    lens = np.diff(raw.indptr)
    assert raw.shape == (N, K) and set(lens) == set(LENGTHS)
    rid = R.row_ids(raw.indptr)
    eng = _lib.Engine(gpu_device)
    eng.set_option('report_kernel', 0)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), K, score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=3, em_epsilon=0.0))
    tl._raw = raw
    tl.em()
    pi, theta = eng.get_params(_lib.Z_CUR)
    eng.set_params(pi, theta)
    want = _oracle(raw, pi, theta)
    nb0 = want[R.INITIAL][0]
    assert np.any((nb0 > 1) & (lens <= 64)) and np.any((nb0 > 1) & (lens > 64)) and nb0.max() > 64     # ties on both sides, wide ones too
    rng = np.random.RandomState(5)
    listed = rng.permutation(N)[:2 * N // 3].astype(np.int32)         # a shuffled row list
    in_list = np.zeros(N, bool); in_list[listed] = True
    group = rng.randint(-1, GROUPS, N).astype(np.int32)               # (-1: a row of no group)

    def colsum(vals, keep=None):
        sel = np.ones(raw.nnz, bool) if keep is None else keep[rid]
        return np.bincount(raw.indices[sel], weights=vals[sel], minlength=K)

    for reproducible in (0, 1):
        eng.set_option('reproducible', reproducible)
        for which, dev in ((R.INITIAL, _lib.Z_INITIAL), (R.CUR, _lib.Z_CUR)):
            nb, picks, assigned = want[which]
            what = 'reproducible %d, %s z' % (reproducible, which)
            assert np.array_equal(eng.best_counts(dev), nb), what
            tr, tc = eng.best_ties(dev)
            assert np.array_equal(tr, np.flatnonzero(nb > 1)) and np.array_equal(tc, nb[nb > 1]), what
            sums, rr, rc = eng.report_colsums(dev, THRESH)
            assert np.array_equal(rr, tr) and np.array_equal(rc, tc), what
            for m in ('exclude', 'average', 'conf'):
                _same(sums[m], colsum(assigned[m]), m, what + ', report_colsums')
            for m in R.METHODS:
                pk = picks if m == 'choose' else None
                cs, mask = eng.reassign(m, THRESH, dev, pk, want_mask=True)
                _same(mask, assigned[m], m, what + ', reassign mask')
                _same(cs, colsum(assigned[m]), m, what + ', reassign column sums')
                got = eng.reassign_rows(m, THRESH, dev, listed, None if pk is None else pk[listed])
                _same(got, colsum(assigned[m], in_list), m, what + ', reassign_rows')
                got = eng.reassign_groups(m, THRESH, dev, group, GROUPS, pk)
                for g in range(GROUPS):
                    _same(got[g], colsum(assigned[m], group == g), m, what + ', reassign_groups, group %d' % g)
    eng.close()
