"""Plain references of the csr_matrix_plus arithmetic (sparse_plus.py: norm, scale, binmax) on `(indptr, data, n_cols)`, and the
seeded inputs that tests/test_csr_reference.py (CPU: these references against the oracle's scipy restatements) and
tests/test_gpu_csr_primitives.py (GPU: the HIP kernels against these references) share.

numpy, math.fsum and np.longdouble only: nothing here imports telescope_amd, so the references owe nothing to the kernels.

Maxima are numpy's (`np.maximum`: a NaN stays), with an implicit 0 where a row (a matrix) holds fewer entries than it has
columns (cells), as scipy's `max` has it.  Sums are exact (`math.fsum`: the correctly rounded sum, one rounding); the quotient of
the two sum-based operations is formed in long double, so the reference adds no fp64 rounding of its own to it.
"""
import math

import numpy as np

U = 2.0 ** -53                                  # unit roundoff of fp64
assert np.finfo(np.longdouble).eps < 2.0 ** -60, 'np.longdouble is not wider than fp64 here: the sum references need it'


def recip0(v):
    """1 / v with inf -> 0 (sparse_plus.py:16-22, oracle/telescope_oracle.py:37)."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(divide='ignore'):
        r = 1.0 / v
    r[np.isinf(r)] = 0
    return r


def row_ids(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def row_max(indptr, data, n_cols):
    """Per row: the maximum of the stored values and, when the row has fewer than n_cols of them, 0."""
    lens = np.diff(indptr)
    m = np.zeros(len(lens))
    full = lens > 0
    if full.any():
        m[full] = np.maximum.reduceat(data, indptr[:-1][full])
    short = full & (lens < n_cols)
    m[short] = np.maximum(m[short], 0.0)
    return m


def ref_binmax(indptr, data, n_cols):
    return (data == row_max(indptr, data, n_cols)[row_ids(indptr)]).astype(np.int8)


def ref_scale_rows(indptr, data, n_cols):
    return data * recip0(row_max(indptr, data, n_cols))[row_ids(indptr)]


def all_max(indptr, data, n_cols):
    m = np.maximum.reduce(data)
    if len(data) < (len(indptr) - 1) * n_cols:
        m = np.maximum(m, 0.0)
    return m


def ref_scale_all(indptr, data, n_cols):
    """scale(): data * (1 / max), no recip0 (sparse_plus.py:94-95).  Needs at least one stored value."""
    with np.errstate(divide='ignore', invalid='ignore'):
        return data * (1.0 / np.float64(all_max(indptr, data, n_cols)))


def row_sums(indptr, data):
    """Exact row sums, correctly rounded to fp64."""
    d = data.tolist()
    ip = indptr.tolist()
    return np.array([math.fsum(d[ip[i]:ip[i + 1]]) for i in range(len(ip) - 1)], dtype=np.float64)


def ref_norm_rows(indptr, data, f64=False):
    """norm(1).  f64=False: data / S in long double (S exact: what the tolerance `sum_bound` is taken against);
    f64=True: the fp64 form data * recip0(S), which is the expected BITS whenever every sum is exact in fp64.
    A zero sum gives zeros (recip0)."""
    s = row_sums(indptr, data)
    if f64:
        return data * recip0(s)[row_ids(indptr)]
    sl = s.astype(np.longdouble)[row_ids(indptr)]
    out = np.zeros(len(data), dtype=np.longdouble)
    nz = sl != 0
    out[nz] = data.astype(np.longdouble)[nz] / sl[nz]
    return out


def ref_norm_all(data, f64=False):
    """norm(): as ref_norm_rows with one sum over all the data, but with a plain 1 / S (sparse_plus.py:47-48 has no recip0 here,
    nor has oracle.norm): a zero sum gives inf / NaN in the fp64 form, and is not taken in long double."""
    s = np.float64(math.fsum(data.tolist()))
    if f64:
        with np.errstate(divide='ignore', invalid='ignore'):
            return data * (1.0 / s)
    assert s != 0
    return data.astype(np.longdouble) / np.longdouble(s)


def sum_bound(ref, n):
    """|got - ref| <= (n + 3) u |ref| for a sum of n non-negative terms added in ANY order: (n - 1) u for the additions, one
    rounding each for the kernel's reciprocal and product and for fsum's result, one u for second-order terms and long double."""
    return (np.asarray(n, dtype=np.longdouble) + 3) * np.longdouble(U) * np.abs(ref)


def sum_error_fraction(got, ref, n):
    """Largest |got - ref| as a fraction of sum_bound (0 where both are 0).  `n` a scalar or one count per element."""
    err = np.abs(got.astype(np.longdouble) - ref)
    bound = sum_bound(ref, n)
    frac = np.zeros(len(err), dtype=np.longdouble)
    nz = bound > 0
    frac[nz] = err[nz] / bound[nz]
    frac[~nz & (err > 0)] = np.inf
    return float(frac.max()) if len(frac) else 0.0


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
# Value legs.  The integer-valued ones make every sum exact in fp64 (|sum| <= 5e6 * 1000 < 2^53): all five operations are then
# compared bit for bit, norm included, whatever the order of additions.  The float ones are non-negative: the sum bound needs it.
INT_LEGS = ('int_pos', 'int_mixed', 'int_neg')
FLOAT_LEGS = ('uniform', 'wide')
LEGS = INT_LEGS + FLOAT_LEGS
_INT_RANGE = {'int_pos': (1, 1000), 'int_mixed': (-1000, 1000), 'int_neg': (-1000, -1)}
ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 255, 256, 257, 1000, 5000)


def _seed(*key):
    """A seed from names and numbers (not hash(): that one changes from process to process)."""
    s = 0
    for ch in repr(key).encode():
        s = (s * 131 + ch) % (2 ** 32 - 5)
    return s


def values(leg, n, rng):
    """n values of a leg.  Integer legs stay one short of their upper end (`top` is planted as a strict maximum)."""
    if leg in _INT_RANGE:
        lo, hi = _INT_RANGE[leg]
        v = rng.randint(lo, hi, size=n).astype(np.float64)            # [lo, hi - 1]: stored zeros occur in int_mixed
        few = rng.randint(lo, min(lo + 4, hi), size=n)                # half the values from four neighbours: many exact ties
        return np.where(rng.rand(n) < 0.5, few, v).astype(np.float64)
    if leg == 'uniform':
        return 0.5 + 0.5 * rng.random_sample(n)
    if leg == 'wide':
        return 2.0 ** rng.uniform(-20.0, 0.0, n)
    raise KeyError(leg)


def top(leg):
    """A value above everything `values` draws: the planted maximum of scale(), the dominant term of norm() (2^30 exceeds the sum
    of 2^23 values below 1, so losing it changes every output grossly; it is non-negative, so the sum bound holds)."""
    return float(_INT_RANGE[leg][1]) if leg in _INT_RANGE else 2.0 ** 30


def plant_row_ties(indptr, data):
    """In every second row, copy the row's maximum to its first and last entry and to entries 16 and 33 where the row has them:
    ties that sit in different lanes of a 16-lane row pass and in different trips of its loop (value ranges are unchanged)."""
    lens = np.diff(indptr)
    sel = np.nonzero((lens > 1) & (np.arange(len(lens)) % 2 == 1))[0]
    if not len(sel):
        return
    m = np.maximum.reduceat(data, indptr[:-1][lens > 0])
    m_of = np.zeros(len(lens))
    m_of[lens > 0] = m
    for off in (0, 16, 33, -1):
        rows = sel if off <= 0 else sel[lens[sel] > off]
        pos = indptr[rows] + off if off >= 0 else indptr[rows + 1] - 1
        data[pos] = m_of[rows]


def _mixed_lengths(rng):
    body = np.array(ROW_LENGTHS[1:] * 3)
    rng.shuffle(body)
    cut = len(body) // 2
    return np.concatenate([[0, 0], body[:cut], [0, 0, 0], body[cut:cut + 5], [0], body[cut + 5:], [0]])


# name -> (row lengths from a seeded rng, columns for "a longest row is dense").  Row counts straddle one sweep of a grid of
# 8192 blocks x 16 rows, and more than two sweeps; their rows are short (0 .. 32 entries), about 16 per row.
ROW_SHAPES = {'lengths_mixed': lambda rng: _mixed_lengths(rng)}
for _n in (1, 15, 16, 17, 131071, 131072, 131073, 300000):
    ROW_SHAPES['rows_%d' % _n] = (lambda n: lambda rng: rng.randint(0, 33, size=n))(_n)
for _l in (1, 3, 15, 16, 17, 33, 257):
    ROW_SHAPES['dense_len_%d' % _l] = (lambda l: lambda rng: np.full(37, l))(_l)
LARGE_ROW_SHAPES = ('rows_131071', 'rows_131072', 'rows_131073', 'rows_300000')


def row_case(shape, leg):
    """(indptr, data, n_cols_dense): a seeded matrix of ROW_SHAPES[shape] with values of `leg`.  With n_cols_dense columns the
    longest rows have no implicit zero; with more, every row has one."""
    rng = np.random.RandomState(_seed('row', shape, leg))
    lens = np.asarray(ROW_SHAPES[shape](rng), dtype=np.int64)
    if shape == 'rows_1':
        lens[:] = 19
    elif shape.startswith('rows_'):
        lens[-1] = lens.max()           # the last row is full: an all-negative short row scales to zeros, which unwritten memory may hold
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    data = values(leg, int(indptr[-1]), rng)
    plant_row_ties(indptr, data)
    return indptr, data, int(max(1, lens.max()))


FLAT_NNZ = (1, 255, 256, 257, 131071, 131072, 131073, 5000003)
LARGE_FLAT_NNZ = (5000003,)


def flat_plants(nnz):
    """Where the maximum / dominant term goes: first, last, and the first element of the second trip of a 512 x 256 thread loop."""
    return sorted({0, nnz - 1} | ({131072} if nnz > 131072 else set()))


def flat_case(nnz, leg, plant):
    """(indptr, data): one row of nnz values of `leg` with top(leg) at index `plant`.  Modes 0 and 1 of tsem_csr_scale read only
    indptr[n_rows] and n_rows * n_cols, so the one row stands for any matrix of nnz entries."""
    rng = np.random.RandomState(_seed('flat', nnz, leg, plant))
    data = values(leg, nnz, rng)
    data[plant] = top(leg)
    return np.array([0, nnz], dtype=np.int64), data


def columns(indptr):
    """Column ids 0, 1, 2, .. within each row: what turns (indptr, data) into a scipy matrix for the oracle."""
    return (np.arange(indptr[-1]) - np.repeat(indptr[:-1], np.diff(indptr))).astype(np.int64)


# Non-finite values, hand-written (4 columns): NaN alone, NaN beside a larger finite value (short and full row), +inf, -inf,
# [inf, 1], a full row of finite values for contrast, an empty row.
NONFINITE_ROWS = ([np.nan], [1.0, np.nan], [np.nan, 7.0, 3.0, 2.0], [np.inf], [-np.inf], [np.inf, 1.0], [-np.inf, -1.0, -2.0, -3.0],
                  [4.0, 3.0, 2.0, 1.0], [], [2.0, np.inf, 5.0, np.inf])


def nonfinite_case(rows=NONFINITE_ROWS):
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return indptr, np.array([v for r in rows for v in r], dtype=np.float64), 4
