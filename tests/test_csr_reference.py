"""CPU side of the csr_matrix_plus primitive tests (tests/test_gpu_csr_primitives.py is the GPU side).

1. The references of tests/_csr_reference.py against the oracle's scipy restatements (oracle.telescope_oracle.norm / scale /
   binmax_rows), on the inputs the GPU tests use (the largest shapes thinned): maxima-based results bit-equal, sum-based results
   within (n + 3) * 2^-53.  So the tolerance the kernels are held to holds for scipy itself against the same reference.
2. The argument checks of tsem_csr_norm_rows / tsem_csr_binmax_rows / tsem_csr_scale.  They run on the host before the device is
   touched, so malformed row pointers are refused identically with and without a GPU, and no test ever sends them to one.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import _csr_reference as R
from oracle import telescope_oracle as O
from telescope_amd import _lib


def as_scipy(indptr, data, n_cols):
    return sp.csr_matrix((data, R.columns(indptr), indptr), shape=(len(indptr) - 1, n_cols))


def dense_marks(marks, indptr, n_cols):
    """int8 marks on the input pattern -> dense array (what oracle.binmax_rows(...).toarray() is compared with)."""
    return as_scipy(indptr, marks, n_cols).toarray()


def check_against_oracle(indptr, data, n_cols, leg, tag, rows=True):
    """Every operation of the reference against the oracle on one matrix; returns the largest sum error as a fraction of the bound."""
    m = as_scipy(indptr, data, n_cols)
    lens = np.diff(indptr)
    worst = 0.0
    with np.errstate(all='ignore'):                      # (1 / 0 and 0 * inf are part of what is compared)
        if rows:
            assert np.array_equal(O.binmax_rows(m).toarray(), dense_marks(R.ref_binmax(indptr, data, n_cols), indptr, n_cols)), (tag, 'binmax')
            np.testing.assert_array_equal(O.scale(m, 1).toarray(), as_scipy(indptr, R.ref_scale_rows(indptr, data, n_cols), n_cols).toarray(),
                                          err_msg='%s scale(1)' % (tag,))
            got = O.norm(m, 1)
            assert np.array_equal(got.indptr, indptr)
            if leg in R.INT_LEGS:
                assert np.array_equal(got.data, R.ref_norm_rows(indptr, data, f64=True)), (tag, 'norm(1)')
            else:
                f = R.sum_error_fraction(got.data, R.ref_norm_rows(indptr, data), np.repeat(lens, lens))
                assert f <= 1.0, (tag, 'norm(1)', f)
                worst = max(worst, f)
        if len(data):
            np.testing.assert_array_equal(O.scale(m).data, R.ref_scale_all(indptr, data, n_cols), err_msg='%s scale()' % (tag,))
            got = O.norm(m)
            if leg in R.INT_LEGS:
                np.testing.assert_array_equal(got.data, R.ref_norm_all(data, f64=True), err_msg='%s norm()' % (tag,))
            else:
                f = R.sum_error_fraction(got.data, R.ref_norm_all(data), len(data))
                assert f <= 1.0, (tag, 'norm()', f)
                worst = max(worst, f)
    return worst


# the largest shapes in two legs (an exact and a rounded one), the very largest in one, instead of in all five: this is the CPU suite
ROW_PARAMS = [(s, l) for s in sorted(R.ROW_SHAPES) for l in R.LEGS
              if s not in R.LARGE_ROW_SHAPES or (l in ('int_mixed', 'wide') if s != R.LARGE_ROW_SHAPES[-1] else l == 'wide')]
FLAT_PARAMS = [(n, l) for n in R.FLAT_NNZ for l in R.LEGS if n not in R.LARGE_FLAT_NNZ or l in ('int_mixed', 'wide')]


@pytest.mark.parametrize('shape,leg', ROW_PARAMS)
def test_row_references_match_the_oracle(shape, leg):
    indptr, data, k = R.row_case(shape, leg)
    worst = max(check_against_oracle(indptr, data, kk, leg, (shape, leg, kk)) for kk in (k, k + 3))
    print('%s %s: scipy sum error %.3g of the bound' % (shape, leg, worst))


@pytest.mark.parametrize('nnz,leg', FLAT_PARAMS)
def test_flat_references_match_the_oracle(nnz, leg):
    worst = 0.0
    for plant in R.flat_plants(nnz):
        indptr, data = R.flat_case(nnz, leg, plant)
        for k in (nnz, nnz + 1):
            worst = max(worst, check_against_oracle(indptr, data, k, leg, (nnz, leg, plant, k), rows=False))
    print('nnz %d %s: scipy sum error %.3g of the bound' % (nnz, leg, worst))


def test_nonfinite_maxima_match_the_oracle():
    """NaN stays in a maximum (np.maximum), also next to a larger finite value and next to the implicit zero."""
    indptr, data, k = R.nonfinite_case()
    m = as_scipy(indptr, data, k)
    assert np.array_equal(O.binmax_rows(m).toarray(), dense_marks(R.ref_binmax(indptr, data, k), indptr, k))
    with np.errstate(invalid='ignore'):
        np.testing.assert_array_equal(O.scale(m, 1).toarray(), as_scipy(indptr, R.ref_scale_rows(indptr, data, k), k).toarray())
        np.testing.assert_array_equal(O.scale(m).data, R.ref_scale_all(indptr, data, k))
    assert np.isnan(R.ref_scale_all(indptr, data, k)).all()
    assert list(R.ref_binmax(indptr, data, k)[:6]) == [0, 0, 0, 0, 0, 0]       # rows [nan], [1, nan], [nan, 7, 3, 2]: nothing marked


def test_known_answers_of_the_edges():
    """scipy's answers for the sign / implicit-zero edges, written out."""
    ip = np.array([0, 3], dtype=np.int64)
    d = np.array([-5.0, -6.0, -7.0])
    assert np.array_equal(R.ref_scale_rows(ip, d, 3), d * (1.0 / -5.0)) and np.allclose(R.ref_scale_rows(ip, d, 3), [1, 1.2, 1.4])
    assert list(R.ref_binmax(ip, d, 3)) == [1, 0, 0]
    assert np.array_equal(R.ref_scale_rows(ip, d, 4), [0, 0, 0]) and list(R.ref_binmax(ip, d, 4)) == [0, 0, 0]
    assert list(R.ref_binmax(np.array([0, 1]), np.array([0.0]), 5)) == [1]      # a lone stored zero is marked
    assert np.array_equal(R.ref_scale_all(ip, d, 4), [-np.inf] * 3)
    for k in (3, 4):
        check_against_oracle(ip, d, k, 'int_neg', ('neg', k))
    check_against_oracle(np.array([0, 1], dtype=np.int64), np.array([0.0]), 5, 'int_mixed', 'zero')


# ---- argument validation (host, before the device) ------------------------------------------------------------------------------
BAD_INDPTR = {'non_monotone': [0, 10, 5], 'first_not_zero': [3, 5], 'negative': [0, -1]}


def _wrappers():
    return {'norm_rows': lambda ip, d: _lib.csr_norm_rows(ip, d),
            'binmax_rows': lambda ip, d: _lib.csr_binmax_rows(ip, d, 16),
            'scale_0': lambda ip, d: _lib.csr_scale(0, ip, d, 16),
            'scale_1': lambda ip, d: _lib.csr_scale(1, ip, d, 16),
            'scale_2': lambda ip, d: _lib.csr_scale(2, ip, d, 16)}


@pytest.fixture(scope='module')
def built():
    _lib.build_library()
    return _lib.lib()


@pytest.mark.parametrize('entry', sorted(_wrappers()))
@pytest.mark.parametrize('bad', sorted(BAD_INDPTR))
def test_malformed_row_pointers_are_refused_on_the_host(built, bad, entry):
    """TSEM_ERR_ARG (-1) with a text, from the host scan: the same with and without a GPU, because the scan comes before
    hipSetDevice.  The data array is as long as the largest row pointer, so even an unchecked read would stay inside it."""
    ip = np.array(BAD_INDPTR[bad], dtype=np.int64)
    with pytest.raises(_lib.EngineError) as e:
        _wrappers()[entry](ip, np.ones(16))
    assert e.value.code == -1, str(e.value)
    assert 'indptr' in str(e.value)


def test_other_bad_arguments_are_refused_on_the_host(built):
    vp = ctypes.c_void_p
    ip = np.array([0, 2], dtype=np.int64)
    d, o, ob = np.ones(2), np.zeros(2), np.zeros(2, np.int8)
    P = _lib.ptr
    calls = {
        'n_rows < 0': lambda: built.tsem_csr_norm_rows(0, -1, P(ip), P(d), P(o)),
        'n_cols < 0': lambda: built.tsem_csr_binmax_rows(0, 1, -1, P(ip), P(d), P(ob)),
        'n_cols < 0 (scale)': lambda: built.tsem_csr_scale(0, 2, 1, -1, P(ip), P(d), P(o)),
        'indptr NULL': lambda: built.tsem_csr_norm_rows(0, 1, vp(None), P(d), P(o)),
        'data NULL': lambda: built.tsem_csr_norm_rows(0, 1, P(ip), vp(None), P(o)),
        'out NULL': lambda: built.tsem_csr_binmax_rows(0, 1, 4, P(ip), P(d), vp(None)),
        'out NULL (scale)': lambda: built.tsem_csr_scale(0, 1, 1, 4, P(ip), P(d), vp(None)),
        'mode': lambda: built.tsem_csr_scale(0, 3, 1, 4, P(ip), P(d), P(o)),
    }
    for what, call in calls.items():
        assert call() == -1, what
        assert built.tsem_last_error(None).decode().startswith('tsem_csr_'), what
