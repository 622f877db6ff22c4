"""The five csr_matrix_plus kernels of telescope_amd/csrc/tsem_csr.hip (k_norm_rows, k_binmax_rows, k_scale_rows, k_reduce_all,
k_scale_all) against references that owe them nothing (tests/_csr_reference.py; tied to scipy by tests/test_csr_reference.py),
at the sizes where such kernels go wrong: rows longer and shorter than a row's lane group, row counts around and beyond one grid
sweep, entry counts around and beyond one trip of the whole-matrix reduction, full rows (no implicit zero) and short ones,
negative values, stored zeros, exact ties across lanes, NaN and infinities, empty rows and matrices.

What is asserted
 * binmax(1), scale(1), scale(): bit for bit, always.  A maximum is exact and `data * (1 / max)` is the same two roundings on both sides.
 * norm(1), norm() on integer-valued data (every sum exact in fp64): bit for bit, whatever the order of additions.
 * norm(1), norm() on non-negative floats: |got - ref| <= (n + 3) * 2^-53 * |ref| against the exact sum (math.fsum) and a long
   double quotient, n = the number of terms.  Derived, not measured: (n - 1) u bounds the additions in ANY order, the kernel's
   reciprocal and product and fsum's result round once each, one more u covers second-order terms and long double.  Each test
   prints the largest error it saw as a fraction of that bound (information; `pytest -s` shows it).
 * non-finite values: scipy's own answers (the oracle), NaN positions included.

Not covered: matrices of more than 2^31 stored entries (17 GB per array; the kernels use 64-bit offsets throughout), sums of
mixed-sign floats (the reference never forms them).  Malformed row pointers are refused on the host and tested there
(tests/test_csr_reference.py): none is ever sent to a GPU.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import _csr_reference as R
from conftest import Opts, case_matrix, load_case
from oracle import telescope_oracle as O
from telescope_amd import _lib
from telescope_amd.sparse_plus import csr_matrix_plus

pytestmark = pytest.mark.gpu


def check_sum_op(got, indptr, data, leg, n, rows, tag):
    """norm(1) (rows=True, n: terms per element) or norm() (n = nnz) under the rules of the module docstring; returns the error fraction."""
    assert got.dtype == np.float64 and got.shape == data.shape, tag
    if leg in R.INT_LEGS:
        want = R.ref_norm_rows(indptr, data, f64=True) if rows else R.ref_norm_all(data, f64=True)
        np.testing.assert_array_equal(got, want, err_msg=str(tag))
        return 0.0
    ref = R.ref_norm_rows(indptr, data) if rows else R.ref_norm_all(data)
    f = R.sum_error_fraction(got, ref, n)
    assert f <= 1.0, '%s: error is %.4g of the bound (n + 3) * 2^-53 * |ref|' % (tag, f)
    return f


def check_whole_matrix_ops(indptr, data, n_cols, leg, tag):
    if not len(data):
        return 0.0
    got = _lib.csr_scale(1, indptr, data, n_cols)
    np.testing.assert_array_equal(got, R.ref_scale_all(indptr, data, n_cols), err_msg='%s scale()' % (tag,))
    return check_sum_op(_lib.csr_scale(0, indptr, data, n_cols), indptr, data, leg, len(data), False, (tag, 'norm()'))


@pytest.mark.parametrize('leg', R.LEGS)
@pytest.mark.parametrize('shape', sorted(R.ROW_SHAPES))
def test_row_kernels(gpu_device, shape, leg):
    """Every element of every operation, with as many columns as the longest row has entries (that row is full: no implicit zero)
    and with three more (every row has one)."""
    indptr, data, k = R.row_case(shape, leg)
    lens = np.diff(indptr)
    worst = check_sum_op(_lib.csr_norm_rows(indptr, data), indptr, data, leg, np.repeat(lens, lens), True, (shape, leg, 'norm(1)'))
    for n_cols in (k, k + 3):
        tag = (shape, leg, 'n_cols=%d' % n_cols)
        got = _lib.csr_binmax_rows(indptr, data, n_cols)
        assert got.dtype == np.int8
        assert np.array_equal(got, R.ref_binmax(indptr, data, n_cols)), (tag, 'binmax(1)')
        assert np.array_equal(_lib.csr_scale(2, indptr, data, n_cols), R.ref_scale_rows(indptr, data, n_cols)), (tag, 'scale(1)')
        worst = max(worst, check_whole_matrix_ops(indptr, data, n_cols, leg, tag))
    print('%s %s: %d rows, %d entries, largest sum error %.3g of the bound' % (shape, leg, len(lens), len(data), worst))


@pytest.mark.parametrize('leg', R.LEGS)
@pytest.mark.parametrize('nnz', R.FLAT_NNZ)
def test_whole_matrix_kernels(gpu_device, nnz, leg):
    """norm() and scale() with the maximum / the dominant term planted first, last and at 131 072, on a full matrix
    (nnz == n_rows * n_cols: no implicit zero) and on one with a single empty cell."""
    worst = 0.0
    for plant in R.flat_plants(nnz):
        indptr, data = R.flat_case(nnz, leg, plant)
        for n_cols in (nnz, nnz + 1):
            worst = max(worst, check_whole_matrix_ops(indptr, data, n_cols, leg, (nnz, leg, 'plant=%d' % plant, 'n_cols=%d' % n_cols)))
    print('nnz %d %s: largest sum error %.3g of the bound' % (nnz, leg, worst))


def as_scipy(indptr, data, n_cols):
    return sp.csr_matrix((data, R.columns(indptr), indptr), shape=(len(indptr) - 1, n_cols))


def check_against_scipy(indptr, data, n_cols, tag):
    """All five operations against the oracle, NaN positions included (tiny matrices: dense comparison)."""
    m = as_scipy(indptr, data, n_cols)
    with np.errstate(all='ignore'):
        np.testing.assert_array_equal(as_scipy(indptr, _lib.csr_norm_rows(indptr, data), n_cols).toarray(), O.norm(m, 1).toarray(),
                                      err_msg='%s norm(1)' % (tag,))
        np.testing.assert_array_equal(as_scipy(indptr, _lib.csr_scale(2, indptr, data, n_cols), n_cols).toarray(), O.scale(m, 1).toarray(),
                                      err_msg='%s scale(1)' % (tag,))
        np.testing.assert_array_equal(as_scipy(indptr, _lib.csr_binmax_rows(indptr, data, n_cols), n_cols).toarray(),
                                      O.binmax_rows(m).toarray(), err_msg='%s binmax(1)' % (tag,))
        np.testing.assert_array_equal(_lib.csr_scale(0, indptr, data, n_cols), O.norm(m).data, err_msg='%s norm()' % (tag,))
        np.testing.assert_array_equal(_lib.csr_scale(1, indptr, data, n_cols), O.scale(m).data, err_msg='%s scale()' % (tag,))


def test_nonfinite_values_follow_scipy(gpu_device):
    """NaN alone in a row, NaN beside a larger finite value, +inf, -inf, [inf, 1]: the whole matrix, then every row as a matrix of
    its own, short (implicit zero) and full.  scipy's maximum keeps a NaN: the row of [1, nan] marks nothing and scales to NaN."""
    indptr, data, k = R.nonfinite_case()
    check_against_scipy(indptr, data, k, 'all rows')
    assert list(_lib.csr_binmax_rows(indptr, data, k)[1:3]) == [0, 0]
    assert np.isnan(_lib.csr_scale(2, indptr, data, k)[1:3]).all()
    for i, row in enumerate(R.NONFINITE_ROWS):
        ip, d, _ = R.nonfinite_case([row])
        for n_cols in sorted({max(1, len(row)), len(row) + 1}):
            check_against_scipy(ip, d, n_cols, ('row %d' % i, row, n_cols))
    # a NaN far from the maximum of a large matrix: scale() is NaN everywhere, wherever the NaN sits in the reduction
    for pos in (0, 131072, 299999):
        ip, d = R.flat_case(300000, 'uniform', 5)
        d[pos] = np.nan
        assert np.isnan(_lib.csr_scale(1, ip, d, 300000)).all(), pos


def test_sign_and_implicit_zero_edges(gpu_device):
    """scipy's answers, written out: a full row [-5, -6, -7] scales to [1, 1.2, 1.4] and marks its first entry; a short all-negative
    row scales to zeros and marks nothing; a lone stored zero is marked; scale() of an all-negative matrix that is not full is -inf."""
    ip = np.array([0, 3], dtype=np.int64)
    d = np.array([-5.0, -6.0, -7.0])
    assert np.array_equal(_lib.csr_scale(2, ip, d, 3), d * (1.0 / -5.0)) and np.allclose(_lib.csr_scale(2, ip, d, 3), [1, 1.2, 1.4])
    assert list(_lib.csr_binmax_rows(ip, d, 3)) == [1, 0, 0]
    assert np.array_equal(_lib.csr_scale(2, ip, d, 4), [0, 0, 0]) and list(_lib.csr_binmax_rows(ip, d, 4)) == [0, 0, 0]
    assert list(_lib.csr_binmax_rows(np.array([0, 1]), np.array([0.0]), 5)) == [1]
    assert np.array_equal(_lib.csr_scale(1, ip, d, 3), d * (1.0 / -5.0))
    assert np.array_equal(_lib.csr_scale(1, ip, d, 4), [-np.inf] * 3)
    # scale(): a full all-negative matrix (7 x 9), and the same matrix with one entry removed
    rng = np.random.RandomState(11)
    full = -rng.randint(2, 1000, size=63).astype(np.float64)
    full[40] = -1.0
    ipf = np.arange(0, 64, 9, dtype=np.int64)
    assert np.array_equal(_lib.csr_scale(1, ipf, full, 9), full * (1.0 / -1.0))
    less = np.delete(full, 17)
    ipl = ipf.copy(); ipl[2:] -= 1
    assert np.array_equal(_lib.csr_scale(1, ipl, less, 9), np.full(62, -np.inf))
    for a, b, c in ((ipf, full, 9), (ipl, less, 9)):
        check_against_scipy(a, b, c, 'negative 7 x 9')
    # all-zero stored rows, full and short, beside mixed and negative ones; zero row sums of mixed signs; stored zeros in a max
    rows = [[0.0, 0.0, 0.0, 0.0], [0.0, 0.0], [1.0, -1.0], [-3.0, 0.0, -2.0], [2.0, -2.0, 5.0, -5.0], [0.0], [], [-4.0, -4.0, -4.0, -4.0]]
    ip, d, _ = R.nonfinite_case(rows)
    for n_cols in (4, 5):
        check_against_scipy(ip, d, n_cols, 'zeros and signs')
    ip2, d2, _ = R.nonfinite_case([[1.0, -1.0], [0.0]])                      # a zero total: norm() is +-inf and NaN, as in scipy
    check_against_scipy(ip2, d2, 2, 'zero total')


@pytest.mark.parametrize('n_rows', (0, 1, 16, 17, 40))
def test_no_stored_entries(gpu_device, n_rows):
    ip = np.zeros(n_rows + 1, dtype=np.int64)
    d = np.zeros(0)
    assert _lib.csr_norm_rows(ip, d).shape == (0,) and _lib.csr_binmax_rows(ip, d, 7).shape == (0,)
    for mode in (0, 1, 2):
        assert _lib.csr_scale(mode, ip, d, 7).shape == (0,)


# ---- through the class ----------------------------------------------------------------------------------------------------------
def canonical(m):
    m = sp.csr_matrix(m, copy=True)
    m.sum_duplicates()
    m.sort_indices()
    return m


def assert_same_sparse(got, want, tag):
    """Shape, pattern (stored zeros included) and values, NaN positions equal."""
    g, w = canonical(got), canonical(want)
    assert g.shape == w.shape, tag
    assert np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices), (tag, 'pattern')
    np.testing.assert_array_equal(g.data, w.data, err_msg=str(tag))


def random_matrix(n, k, dtype, seed):
    """Random rows of 0 .. 60 entries, plus one full row, one row of a single entry and empty first / last rows."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 61, size=n)
    lens[0] = lens[-1] = 0
    lens[n // 2] = k
    lens[n // 3] = 1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([np.sort(rng.choice(k, l, replace=False)) for l in lens]).astype(np.int32)
    nnz = int(indptr[-1])
    dt = np.dtype(dtype)
    if dt == np.bool_:
        data = np.ones(nnz, dtype=bool)
    elif dt.kind == 'f':
        data = (0.5 + 0.5 * rng.random_sample(nnz)).astype(dt)                # non-negative: the sum bound applies
    else:
        lo = max(np.iinfo(dt).min + 1, -1000)
        data = rng.randint(lo, min(np.iinfo(dt).max, 1000) + 1, size=nnz).astype(dt)
        if dt.kind == 'i':
            data[indptr[n // 2]:indptr[n // 2 + 1]] = -np.abs(data[indptr[n // 2]:indptr[n // 2 + 1]]) - 1   # the full row: all negative
    return sp.csr_matrix((data, indices, indptr), shape=(n, k))


def check_class_against_oracle(m, tag, exact_sums):
    """m: scipy CSR.  The class on m against the oracle on m's canonical fp64 form."""
    mp = csr_matrix_plus(m)
    ref = canonical(m).astype(np.float64)
    worst = 0.0
    with np.errstate(all='ignore'):
        b = mp.binmax(1)
        assert isinstance(b, csr_matrix_plus) and b.dtype == np.int8 and b.shape == m.shape, tag
        assert_same_sparse(b, O.binmax_rows(ref), (tag, 'binmax(1)'))
        for name, got, want in (('scale(1)', mp.scale(1), O.scale(ref, 1)), ('scale()', mp.scale(), O.scale(ref) if ref.nnz else ref)):
            assert isinstance(got, csr_matrix_plus) and got.dtype == np.float64 and got.shape == m.shape, (tag, name)
            assert_same_sparse(got, want, (tag, name))
        lens = np.diff(ref.indptr)
        for name, got, want, n, rows in (('norm(1)', mp.norm(1), O.norm(ref, 1), np.repeat(lens, lens), True),
                                         ('norm()', mp.norm(), O.norm(ref), ref.nnz, False)):
            assert isinstance(got, csr_matrix_plus) and got.dtype == np.float64 and got.shape == m.shape, (tag, name)
            if exact_sums:
                assert_same_sparse(got, want, (tag, name))
            else:
                g = canonical(got)
                assert np.array_equal(g.indptr, ref.indptr) and np.array_equal(g.indices, ref.indices), (tag, name, 'pattern')
                worst = max(worst, check_sum_op(g.data, ref.indptr, ref.data, 'float', n, rows, (tag, name)))
    return worst


@pytest.mark.parametrize('dtype', ('bool', 'int8', 'uint16', 'int32', 'int64', 'float32', 'float64'))
def test_class_dtypes(gpu_device, dtype):
    """Every input dtype gives int8 from binmax and float64 from the rest, with the oracle's values.  float32 is the one known
    difference from the reference: scipy keeps float32 there, the class computes and returns float64 (sparse_plus.py docstring);
    its values are those of the oracle on the input cast to float64."""
    m = random_matrix(4000, 3000, dtype, seed=5)
    assert m.dtype == np.dtype(dtype)
    worst = check_class_against_oracle(m, dtype, exact_sums=np.dtype(dtype).kind != 'f')
    if dtype == 'float32':
        assert O.norm(m, 1).dtype == np.float32 and csr_matrix_plus(m).norm(1).dtype == np.float64
    print('%s: largest sum error %.3g of the bound' % (dtype, worst))


def test_class_canonicalises_duplicates_and_unsorted_indices(gpu_device):
    rng = np.random.RandomState(9)
    n, k = 3000, 500
    lens = rng.randint(0, 40, size=n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = rng.randint(0, 25, size=indptr[-1]).astype(np.int32)           # 0 .. 39 draws from 25 columns: duplicates, unsorted
    data = rng.randint(-50, 51, size=indptr[-1]).astype(np.float64)
    m = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    assert not m.has_canonical_format and canonical(m).nnz < m.nnz
    check_class_against_oracle(m, 'duplicates', exact_sums=True)
    assert m.nnz == len(data) and np.array_equal(m.indices, indices)         # the caller's matrix is left as it was


def test_class_keeps_explicit_zeros(gpu_device):
    """Stored zeros keep their place in norm / scale and are dropped by binmax (eliminate_zeros, as oracle.binmax_rows does) —
    unless the zero IS the row maximum: then it is marked."""
    m = random_matrix(2000, 300, 'int32', seed=13)
    m.data[::3] = 0
    mp = csr_matrix_plus(m)
    check_class_against_oracle(m, 'stored zeros', exact_sums=True)
    for r in (mp.norm(1), mp.scale(1), mp.scale(), mp.norm()):
        assert r.nnz == m.nnz and np.array_equal(r.indices, m.indices) and np.array_equal(r.indptr, m.indptr)
    b = mp.binmax(1)
    assert b.nnz < m.nnz and (b.data == 1).all()
    z = csr_matrix_plus(sp.csr_matrix((np.array([0.0, -2.0]), np.array([1, 3]), np.array([0, 2])), shape=(1, 2 + 3)))
    assert np.array_equal(z.binmax(1).toarray(), [[0, 1, 0, 0, 0]])


def test_class_empty_matrices(gpu_device):
    """(3, 4) and (0, 5) without entries, one row of stored zeros: the oracle's results, no error.  One difference is pinned: scipy's
    `max()` of a matrix with a zero dimension raises ValueError, so oracle.scale() of (0, 5) does; the class returns the empty matrix."""
    for shape in ((3, 4), (0, 5)):
        m = sp.csr_matrix(shape, dtype=np.float64)
        mp = csr_matrix_plus(m)
        for name, got, want in (('norm()', mp.norm(), lambda: O.norm(m)), ('norm(1)', mp.norm(1), lambda: O.norm(m, 1)),
                                ('scale(1)', mp.scale(1), lambda: O.scale(m, 1)), ('binmax(1)', mp.binmax(1), lambda: O.binmax_rows(m)),
                                ('scale()', mp.scale(), lambda: O.scale(m))):
            assert got.shape == shape and got.nnz == 0 and got.dtype == (np.int8 if name == 'binmax(1)' else np.float64), (shape, name)
            if (shape, name) == ((0, 5), 'scale()'):
                with pytest.raises(ValueError):
                    want()
            else:
                with np.errstate(all='ignore'):
                    assert_same_sparse(got, want(), (shape, name))
    zero_row = sp.csr_matrix((np.zeros(3), np.array([0, 1, 2]), np.array([0, 3])), shape=(1, 3))
    check_class_against_oracle(zero_row, 'zero row, full', exact_sums=True)
    check_class_against_oracle(sp.csr_matrix((np.zeros(3), np.array([0, 1, 2]), np.array([0, 3])), shape=(1, 4)), 'zero row, short', exact_sums=True)
    assert np.array_equal(csr_matrix_plus(zero_row).binmax(1).toarray(), [[1, 1, 1]])


@pytest.mark.parametrize('case', ('bundled', 'tiny_ties', 'tiny_twins', 'tiny_empty_row'))
def test_reassign_rebuilt_from_the_class(gpu_device, case):
    """The reference builds `reassign` from these primitives (model.py:837-856); the engine has fused report kernels instead.  On
    the engine's own z (exact ties included) the two must agree: exclude and choose exactly, average bit for bit (its sums are
    counts and 1 * (1 / c) is the same expression on both sides), conf in pattern, with every entry within 2 ulp of 1."""
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case(case)
    tl = TelescopeLikelihood(case_matrix(c), Opts(c), device=gpu_device)
    tl.em()
    z = csr_matrix_plus(tl.z)
    v = z.binmax(1)
    exclude = sp.csr_matrix(v.multiply(v.sum(1) == 1))
    assert_same_sparse_values(exclude, tl.reassign('exclude').tocsr(), (case, 'exclude'))
    np.random.seed(20240229)
    choose = v.choose_random(1)
    np.random.seed(20240229)
    assert_same_sparse_values(choose, tl.reassign('choose').tocsr(), (case, 'choose'))
    assert_same_sparse_values(v.norm(1), tl.reassign('average').tocsr(), (case, 'average'))
    conf = z.apply_func(lambda x: x if x >= 0.9 else 0).norm(1)
    got, want = canonical(conf), canonical(tl.reassign('conf').tocsr())
    got.eliminate_zeros(); want.eliminate_zeros()
    assert np.array_equal(got.indptr, want.indptr) and np.array_equal(got.indices, want.indices), (case, 'conf pattern')
    for d in (got.data, want.data):
        assert np.all(np.abs(d - 1.0) <= 2 * np.spacing(1.0)), (case, 'conf values')


def assert_same_sparse_values(got, want, tag):
    """Equal as matrices (stored zeros do not count), bit for bit."""
    g, w = canonical(got).astype(np.float64), canonical(want).astype(np.float64)
    g.eliminate_zeros(); w.eliminate_zeros()
    assert g.shape == w.shape, tag
    assert np.array_equal(g.indptr, w.indptr) and np.array_equal(g.indices, w.indices), (tag, 'pattern')
    assert np.array_equal(g.data, w.data), tag
