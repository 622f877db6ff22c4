"""A plain reference of the row pass's per-entry outputs (k_rowpass of telescope_amd/csrc/tsem_report.hip: the posterior z, the six
reassign masks, the `--updated_sam` tag words), and the seeded inputs that tests/test_rowpass_reference.py (CPU: this reference
against the oracle's scipy restatement) and tests/test_gpu_rowpass_entries.py (GPU: the HIP kernel against this reference) share.

numpy and np.longdouble only for the arithmetic: nothing here touches the engine, so the reference owes nothing to the kernels.
The quantiser of the tag word is `telescope_amd.bam_out.tag_word` / `phred_table` (host numpy, tied to numpy's scalar expressions
in tests/test_rowpass_reference.py); `numpy_z` / `oracle_assigned` come from `oracle.telescope_oracle.OracleModel`, which is pinned
to the reference implementation (tests/test_oracle_golden.py).

Everything is laid out on the stored entries of the raw CSR (`indptr`, `indices`, `raw`): one value per stored entry, in CSR
order, like tsem_export_z.
"""
import numpy as np
import scipy.sparse as sp

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, \
    'np.longdouble has a %d-bit mantissa here: the exact reference of the row pass needs at least 63 bits' % np.finfo(LD).nmant
U = 2.0 ** -53                                  # unit roundoff of fp64
TINY = 2.0 ** -1022                             # smallest normal fp64
METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')
INITIAL, CUR, USER = 'initial', 'cur', 'user'   # sources of z: lut[raw] alone | lut[raw] * (pi theta | pi) | the caller's z
PREV = 'prev'                                   # as CUR, with the parameters of the E-step before the last M-step


def row_ids(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def bound(lens):
    """(len + 3) 2^-53, relative, first order, for z = fl(n_j fl(1 / S)) of a row of `len` stored entries: one rounding each for
    pi * theta (k_cnat), Q * c, 1 / S and n * r, and at most len - 1 for ANY order of adding len positive terms.  Derived from the
    code, same form as tests/_csr_reference.sum_bound; not tuned on a kernel's output."""
    return (np.asarray(lens).astype(LD) + 3) * LD(U)


ABS_SLACK = 2.0 ** -1074
"""Gradual underflow is no relative rounding: where fp64's pi * theta or Q * c is subnormal, `exact_z` takes fp64's value of that
product (both the reference and the kernel hold exactly that number: IEEE multiplication is correctly rounded), and a subnormal
quotient z is given one step of the subnormal grid.  On ordinary data neither ever applies."""


def _row_reduce(ufunc, vals, indptr, empty):
    """ufunc.reduceat over the rows, `empty` for rows without stored entries."""
    lens = np.diff(indptr)
    out = np.full(len(lens), empty, dtype=vals.dtype)
    full = lens > 0
    if full.any():
        out[full] = ufunc.reduceat(vals, indptr[:-1][full])
    return out


def exact_numerators(indptr, indices, raw, lut, pi=None, theta=None, which=CUR, user_z=None):
    """(n, inpat): the numerators of z in long double and z's pattern.
    CUR: lut[raw] * pi[col] * theta[col] for rows with more than one stored entry, lut[raw] * pi[col] for single-entry rows
    (model.py:699-714); INITIAL: lut[raw] (model.py:837); USER: the caller's z as it is (NaN = no entry).
    Pattern (tsem_export_z): an entry whose fp64 numerator is 0 leaves the pattern, except for the initial z."""
    indptr = np.asarray(indptr, dtype=np.int64)
    if which == USER:
        z = np.asarray(user_z, dtype=np.float64)
        inpat = ~np.isnan(z)
        return np.where(inpat, z, 0.0).astype(LD), inpat
    q64 = np.asarray(lut, dtype=np.float64)[raw]
    if which == INITIAL:
        return q64.astype(LD), np.ones(len(q64), dtype=bool)
    pi = np.asarray(pi, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    amb = (np.diff(indptr) > 1)[row_ids(indptr)]
    c64 = pi * theta
    c = pi.astype(LD) * theta.astype(LD)
    sub = np.abs(c64) < TINY                                   # (underflow: see ABS_SLACK)
    c[sub] = c64[sub]
    n64 = q64 * np.where(amb, c64[indices], pi[indices])
    n = q64.astype(LD) * np.where(amb, c[indices], pi.astype(LD)[indices])
    sub = np.abs(n64) < TINY
    n[sub] = n64[sub]
    return n, n64 != 0.0


def exact_z(indptr, indices, raw, lut, pi=None, theta=None, which=CUR, user_z=None):
    """(z, inpat) in long double on the stored entries: numerators as `exact_numerators` has them, row sums with np.add.reduceat
    on long doubles, one long double division.  z is 0 outside the pattern.  The caller's z (USER) is returned as it is.
    Its own error — len additions and a division at 2^-64 — is about len 2^-64: 2^-11 of `bound`."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n, inpat = exact_numerators(indptr, indices, raw, lut, pi, theta, which, user_z)
    if which == USER:
        return n, inpat
    n = np.where(inpat, n, LD(0))
    s = _row_reduce(np.add, n, indptr, LD(0))[row_ids(indptr)]
    z = np.zeros(len(n), dtype=LD)
    with np.errstate(divide='ignore', over='ignore'):
        nz = np.isfinite(1.0 / s.astype(np.float64))               # recip0 (sparse_plus.py:16-22): 1 / S = inf counts as 0, for a zero
    z[nz] = n[nz] / s[nz]                                          # sum and for one so far below the normal range that 1 / S overflows
    return z, inpat


def error_fraction(got, z, inpat, indptr, per_entry=False):
    """|got - z| as a fraction of bound(len) z + ABS_SLACK per entry of the pattern; where z is 0 the limit is 0 (inf for any
    other value: a zero is exact); the largest fraction, or all of them."""
    lens = np.diff(indptr)[row_ids(indptr)]
    err = np.abs(np.asarray(got).astype(LD) - z)
    lim = np.where(z != 0, bound(lens) * np.abs(z) + LD(ABS_SLACK), LD(0))
    frac = np.zeros(len(err), dtype=LD)
    ok = inpat & (lim > 0)
    frac[ok] = err[ok] / lim[ok]
    frac[inpat & (lim == 0) & (err > 0)] = np.inf
    if per_entry:
        return frac
    return float(frac.max()) if len(frac) else 0.0


# ---- the reference's own fp64 operator sequence -----------------------------------------------------------------------------------
def oracle_model(raw, lut):
    """An OracleModel whose Q is `lut[raw]` on raw's pattern (the caller's score table instead of expm1 of the scaled scores;
    stored zeros of Q stay stored, as the device keeps them)."""
    from oracle.telescope_oracle import OracleModel, count_rows
    om = OracleModel.__new__(OracleModel)
    om.raw_scores = raw
    om.N, om.K = raw.shape
    om.Q = sp.csr_matrix((np.asarray(lut, dtype=np.float64)[raw.data], raw.indices.copy(), raw.indptr.copy()), shape=raw.shape)
    om.Y = (count_rows(om.Q) > 1).astype(np.uint8)
    om.z = None
    return om


def align(m, raw, fill=0.0):
    """The values of sparse `m` on raw's stored entries (`fill` where m has no entry there); m's pattern is a subset of raw's."""
    m = sp.csr_matrix(m)
    if m.nnz == raw.nnz and np.array_equal(m.indptr, raw.indptr) and np.array_equal(m.indices, raw.indices):
        return np.asarray(m.data).copy()
    m.sort_indices()
    k = raw.shape[1]
    kq = row_ids(raw.indptr).astype(np.int64) * k + raw.indices
    km = row_ids(m.indptr).astype(np.int64) * k + m.indices
    pos = np.searchsorted(kq, km)
    assert len(km) == 0 or (pos.max() < len(kq) and np.array_equal(kq[pos], km)), 'entries outside the score matrix pattern'
    out = np.full(raw.nnz, fill, dtype=np.result_type(m.dtype, np.float64))
    out[pos] = m.data
    return out


def numpy_z(om, raw, pi=None, theta=None, which=CUR, user_z=None):
    """fp64 z of the reference's operator sequence (OracleModel.estep; norm(Q, 1) for the initial z) on raw's stored entries, 0
    where scipy dropped the entry; also left in `om.z` for `oracle_assigned`."""
    from oracle.telescope_oracle import norm
    if which == USER:
        keep = ~np.isnan(user_z)
        rows = row_ids(raw.indptr)[keep]
        ip = np.zeros(raw.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(rows, minlength=raw.shape[0]), out=ip[1:])
        om.z = sp.csr_matrix((np.asarray(user_z)[keep], raw.indices[keep], ip), shape=raw.shape)
    elif which == INITIAL:
        om.z = norm(om.Q, 1)
    else:
        with np.errstate(over='ignore'):                           # (1 / S of a subnormal row sum: inf, which recip0 turns into 0)
            om.z = om.estep(np.asarray(pi, dtype=np.float64), np.asarray(theta, dtype=np.float64))
    return align(om.z, raw)


class _Picks(object):
    """np.random stand-in for choose_random_rows: the draws are the caller's picks of the rows with several best hits."""
    def __init__(self, draws):
        self.draws = draws

    def randint(self, lo, hi):
        assert len(hi) == len(self.draws) and np.all(self.draws < hi)
        return self.draws


def oracle_best_counts(om, which=CUR):
    from oracle.telescope_oracle import binmax_rows, norm
    return np.diff(binmax_rows(norm(om.Q, 1) if which == INITIAL else om.z).indptr)


def oracle_assigned(om, raw, method, thresh, which=CUR, picks=None):
    """`reassign(method, thresh)` of the oracle (z as the last numpy_z call left it) on raw's stored entries, as float64 values;
    `choose` takes picks[row] (one per row, below the row's number of best hits) where the reference draws."""
    rng = np.random
    if method == 'choose':
        nb = oracle_best_counts(om, which)
        rng = _Picks(np.asarray(picks)[nb > 1])
    return align(om.reassign(method, thresh, initial=(which == INITIAL), rng=rng), raw).astype(np.float64)


# ---- the assignment in exact arithmetic -------------------------------------------------------------------------------------------
def exact_assigned(indptr, z, inpat, thresh, picks=None, methods=METHODS):
    """From exact_z: {method: value per stored entry} for the six methods (model.py:808-865; long double for `average` and `conf`,
    bool for the 0 / 1 methods), the number of best hits per row, and three flags per row.  `clear`: the row's largest z and the
    largest one below it are further apart than 2 bound(len), relative; `clear_thresh`: so is every z of the row from `thresh`.
    On such rows the answer does not depend on rounding: both sides carry z to within bound(len).  `exclude`, `choose`, `average`
    hang on `clear`, `conf` on `clear_thresh`; `unique` and `all` ask for z > 0, which rounding decides only where an exact z lies
    below the subnormal grid (an underflowing quotient: rows with such an entry are not `clear_pos`): see clear_rows."""
    indptr = np.asarray(indptr, dtype=np.int64)
    rid = row_ids(indptr)
    lens = np.diff(indptr)
    zp = np.where(inpat, z, LD(-1))
    zmax = _row_reduce(np.maximum, zp, indptr, LD(-1))
    best = inpat & (zp == zmax[rid])
    nb = np.bincount(rid[best], minlength=len(lens))
    z2 = _row_reduce(np.maximum, np.where(best, LD(-1), zp), indptr, LD(-1))
    b2 = 2 * bound(lens)
    clear = (z2 < 0) | (zmax - z2 > b2 * zmax)
    th = LD(thresh)
    near = inpat & (np.abs(z - th) <= b2[rid] * np.maximum(z, th))
    clear_thresh = np.bincount(rid[near], minlength=len(lens)) == 0
    low = inpat & (z > 0) & (z < LD(4 * ABS_SLACK))
    clear_pos = np.bincount(rid[low], minlength=len(lens)) == 0
    out = {}
    if 'exclude' in methods:
        out['exclude'] = best & (nb[rid] == 1)
    if 'choose' in methods:
        cum = np.cumsum(best) - best                               # ordinal of a best hit, counted over the whole matrix
        first = _row_reduce(np.minimum, np.where(best, cum, np.iinfo(np.int64).max), indptr, 0)
        pk = np.zeros(len(lens), dtype=np.int64) if picks is None else np.where(nb > 1, np.asarray(picks, dtype=np.int64), 0)
        out['choose'] = best & ((cum - first[rid]) == pk[rid])
    if 'average' in methods:
        out['average'] = np.where(best, LD(1) / np.maximum(nb, 1).astype(LD)[rid], LD(0))
    if 'conf' in methods:
        keep = inpat & (z >= th)
        vs = _row_reduce(np.add, np.where(keep, z, LD(0)), indptr, LD(0))[rid]
        out['conf'] = np.where(keep & (vs > 0), z / np.where(vs > 0, vs, LD(1)), LD(0))
    if 'unique' in methods:
        out['unique'] = inpat & (lens[rid] == 1) & (z > 0)         # ceil of a z in (0, 1]
    if 'all' in methods:
        out['all'] = inpat & (z > 0)
    return out, nb, clear, clear_thresh, clear_pos


def clear_rows(method, clear, clear_thresh, clear_pos):
    if method in ('exclude', 'choose', 'average'):
        return clear
    return clear_thresh if method == 'conf' else clear_pos


class Reference(object):
    """Everything a check needs for one (matrix, parameters, source of z): exact z and pattern, the reference's fp64 z, the picks
    `choose` is asked with (one per row, below the oracle's number of best hits), and per method the oracle's values and the exact
    ones with the rows on which they are certain."""

    def __init__(self, raw, lut, pi=None, theta=None, which=CUR, user_z=None, thresh=0.9, seed=0):
        self.raw, self.lut, self.which, self.thresh = raw, np.asarray(lut, dtype=np.float64), which, thresh
        self.pi, self.theta, self.user_z = pi, theta, user_z
        self.indptr = raw.indptr.astype(np.int64)
        self.lens = np.diff(self.indptr)
        self.z, self.inpat = exact_z(self.indptr, raw.indices, raw.data, lut, pi, theta, which, user_z)
        self.om = oracle_model(raw, lut)
        self.zn = numpy_z(self.om, raw, pi, theta, which, user_z)
        self.nbo = nbo = oracle_best_counts(self.om, which)          # best hits per row as the oracle's fp64 z has them
        self.picks = (np.random.RandomState(seed).random_sample(len(self.lens)) * np.maximum(nbo, 1)).astype(np.int32)
        _, self.nb, self.clear, self.clear_thresh, self.clear_pos = exact_assigned(self.indptr, self.z, self.inpat, thresh, methods=())

    def assigned(self, method):
        """(the oracle's value per stored entry, the exact one, the rows where the exact one is certain)"""
        o = oracle_assigned(self.om, self.raw, method, self.thresh, self.which, self.picks)
        e = exact_assigned(self.indptr, self.z, self.inpat, self.thresh, self.picks, methods=(method,))[0][method]
        return o, e, clear_rows(method, self.clear, self.clear_thresh, self.clear_pos)

    def clear_share(self):
        return float(np.mean(self.clear & self.clear_thresh)) if len(self.lens) else 1.0

    def numpy_fraction(self):
        return error_fraction(self.zn, self.z, self.inpat, self.indptr)


# ---- an emulation of the device's order of additions (tsem_report.hip: 16 lane-strided partial sums, then a 4-level tree) ----------
def device_order_z(indptr, n64, inpat):
    """fp64 z = n * (1 / S) with S added like k_rowpass adds it: lane l of 16 adds entries l, l + 16, l + 32, .. in order (rows of up
    to 64 entries: ((n0 + n1) + n2) + n3, the same thing), then a butterfly over the 16 lanes (xor 8, 4, 2, 1; any pairing has the
    same error bound).  n64: fp64 numerators, taken as 0 outside the pattern."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = np.where(inpat, n64, 0.0)
    lens = np.diff(indptr)
    rid = row_ids(indptr)
    pos = np.arange(len(n)) - indptr[:-1][rid]
    part = np.zeros((len(lens), 16))
    for step in range(int((lens.max() + 15) // 16) if len(lens) else 0):
        sel = (pos // 16) == step
        part[rid[sel], pos[sel] % 16] += n[sel]                    # (one entry per (row, lane) and step: no repeated index)
    for w in (8, 4, 2, 1):
        part = part[:, :w] + part[:, w:2 * w]
    s = part[:, 0]
    with np.errstate(divide='ignore'):
        r = 1.0 / s
    r[np.isinf(r)] = 0.0
    return n * r[rid]


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000, 5000)


def _seed(*key):
    s = 0
    for ch in repr(key).encode():
        s = (s * 131 + ch) % (2 ** 32 - 5)
    return s


def matrix_from_lengths(lens, k, max_score, rng, tie_scores=0.3):
    """A uint16 CSR with the given row lengths over k columns: ascending columns at random gaps, scores in [1, max_score]; in a
    share `tie_scores` of the rows the scores come from the two largest values only, so that exact ties between numerators are
    common (with `parameters`, whose columns share values)."""
    lens = np.asarray(lens, dtype=np.int64)
    assert lens.max() <= k
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rid = row_ids(indptr)
    gap = (k // np.maximum(lens, 1))[rid]
    inc = 1 + (rng.random_sample(len(rid)) * gap).astype(np.int64)
    inc = np.minimum(inc, gap)
    cs = np.cumsum(inc)
    start = np.concatenate([[0], cs])[indptr[:-1]]
    indices = (cs - start[rid] - 1).astype(np.int32)
    data = rng.randint(1, max_score + 1, len(rid)).astype(np.uint16)
    few = rng.randint(max(1, max_score - 1), max_score + 1, len(rid)).astype(np.uint16)
    tied = (rng.random_sample(len(lens)) < tie_scores)[rid]
    data = np.where(tied, few, data).astype(np.uint16)
    data[0] = max_score                                             # the largest score occurs: score_lut(max_score) is the model's own table
    m = sp.csr_matrix((data, indices, indptr), shape=(len(lens), k))
    assert m.has_sorted_indices and indices.max(initial=0) < k
    return m


def parameters(k, rng, shared=0.5):
    """Dirichlet pi and theta; a share of the columns takes its pair from a pool of four columns' pairs, so that equal scores give
    EXACT ties (equal inputs give equal numerators in any arithmetic)."""
    pi = rng.dirichlet(np.full(k, 2.0))
    theta = rng.dirichlet(np.full(k, 2.0))
    pool = rng.randint(0, k, 4)
    src = pool[rng.randint(0, 4, k)]
    sel = rng.random_sample(k) < shared
    return np.where(sel, pi[src], pi), np.where(sel, theta[src], theta)


def _mixed_lengths(rng, reps=4, filler=1500):
    body = np.array(EDGE_LENGTHS * reps)
    lens = np.concatenate([body, rng.randint(1, 80, filler)])
    rng.shuffle(lens)
    return lens


SHAPES = {
    'mixed': lambda rng: (_mixed_lengths(rng), 6000),
    'one_row': lambda rng: (np.array([37]), 50),
    'one_column': lambda rng: (np.ones(300, dtype=np.int64), 1),
    'single_first_last': lambda rng: (np.concatenate([[1, 1, 1], rng.randint(2, 70, 500), [1]]), 300),
    'single_only': lambda rng: (np.ones(1000, dtype=np.int64), 40),
    'last_row_longest': lambda rng: (np.concatenate([rng.randint(1, 40, 700), [4999]]), 5200),
    'rows_300000': lambda rng: (rng.randint(1, 17, 300000), 2000),
}
for _l in EDGE_LENGTHS:
    SHAPES['len_%d' % _l] = (lambda l: lambda rng: (np.full(37 if l < 1000 else 5, l), max(l, 8) + l // 3))(_l)


def shape_case(name, max_score=400):
    """(raw, lut, pi, theta) of SHAPES[name], seeded.  max_score 400: the score table fits the LDS (<= 2048 entries); 5000: it
    stays in global memory."""
    from telescope_amd.likelihood import score_lut
    rng = np.random.RandomState(_seed('shape', name, max_score))
    lens, k = SHAPES[name](rng)
    raw = matrix_from_lengths(lens, k, max_score, rng)
    pi, theta = parameters(k, rng)
    return raw, score_lut(max_score), pi, theta


def emulation_matrix(max_score=400, seed=7):
    """The matrix of the emulation check: 20 000 rows of 1 – 79 entries plus 200 rows of 100 – 4999, Dirichlet parameters."""
    from telescope_amd.likelihood import score_lut
    rng = np.random.RandomState(seed)
    lens = np.concatenate([rng.randint(1, 80, 20000), rng.randint(100, 5000, 200)])
    raw = matrix_from_lengths(lens, 6000, max_score, rng, tie_scores=0.0)
    k = raw.shape[1]
    return raw, score_lut(max_score), rng.dirichlet(np.full(k, 2.0)), rng.dirichlet(np.full(k, 2.0))


def dead_column_case(kind, seed=11):
    """Leg (c).  'pi' / 'theta': that parameter is 0 on a fifth of the columns — rows lose some, all but one or all of their
    entries, and the first rows are planted: a two-entry row with one dead column (effectively unique), rows whose columns are all
    dead, a row with one live column; 'denormal': pi * theta is subnormal on a fifth of the columns and underflows to 0 on a few;
    'zero_score_lut0' / 'zero_score': stored scores of 0 with lut[0] == 0 (expm1(0)) and with lut[0] > 0."""
    from telescope_amd.likelihood import score_lut
    rng = np.random.RandomState(_seed('dead', kind, seed))
    k = 400
    lens = np.concatenate([[2, 3, 2, 5, 1, 1], rng.randint(1, 12, 1500), rng.randint(60, 140, 40), [1, 2]])
    raw = matrix_from_lengths(lens, k, 300, rng)
    pi, theta = parameters(k, rng, shared=0.2)
    dead = rng.random_sample(k) < 0.2
    ip, ix = raw.indptr, raw.indices
    dead[ix[ip[0]]] = True; dead[ix[ip[0] + 1]] = False            # row 0: two entries, one dead: effectively unique
    dead[ix[ip[1]:ip[2]]] = True                                    # row 1: every column dead
    dead[ix[ip[0] + 1]] = False
    dead[ix[ip[4]]] = True                                          # row 4: a single-entry row on a dead column
    lut = score_lut(300)
    if kind == 'pi':
        pi = np.where(dead, 0.0, pi)
    elif kind == 'theta':
        theta = np.where(dead, 0.0, theta)                          # (single-entry rows do not read theta: row 4 keeps its entry)
    elif kind == 'denormal':
        pi = np.where(dead, pi * 1e-160, pi)
        theta = np.where(dead, theta * 1e-150, theta)               # products near 1e-315: subnormal
        gone = dead & (rng.random_sample(k) < 0.2)
        theta = np.where(gone, theta * 1e-20, theta)                # and below the subnormal range: 0 in fp64
    elif kind in ('zero_score_lut0', 'zero_score'):
        z = rng.random_sample(raw.nnz) < 0.15
        z[0] = False                                                # (keeps the largest score in the matrix)
        raw = sp.csr_matrix((np.where(z, 0, raw.data).astype(np.uint16), raw.indices, raw.indptr), shape=raw.shape)
        if kind == 'zero_score':
            lut = lut.copy(); lut[0] = 0.25
    else:
        raise KeyError(kind)
    return raw, lut, pi, theta


DEAD_KINDS = ('pi', 'theta', 'denormal', 'zero_score_lut0', 'zero_score')


# ---- near-ties (leg d) ------------------------------------------------------------------------------------------------------------
def near_tie_matrix(seed, n=6000, k=400, max_len=40, long_rows=0, scores=(3, 4)):
    """A matrix whose rows are full of near-ties once the parameters below are set: columns come in PAIRS (2j, 2j + 1) whose
    pi * theta differ by one to three ulp, a row takes both columns of a pair with the same score, so its two largest z values are
    a few ulp apart — whether they round together hangs on the last bit of 1 / rowsum, i.e. on the ORDER the row is added in."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(1, max_len // 2 + 1, n) * 2
    lens[rng.rand(n) < 0.1] = 1
    if long_rows:
        lens[rng.choice(n, long_rows, replace=False)] = rng.choice([130, 258, 300, 398], long_rows)    # beyond the streaming kernel's 256 entries too
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.empty(indptr[-1], np.int32)
    data = np.empty(indptr[-1], np.uint16)
    for i, l in enumerate(lens):
        s = indptr[i]
        if l == 1:
            indices[s] = rng.randint(k); data[s] = rng.choice(scores)
            continue
        pairs = np.sort(rng.choice(k // 2, l // 2, replace=False))
        indices[s:s + l] = np.repeat(2 * pairs, 2) + np.tile([0, 1], l // 2)
        data[s:s + l] = np.repeat(rng.choice(scores, l // 2), 2)
    raw = sp.csr_matrix((data, indices, indptr), shape=(n, k))
    pi = rng.dirichlet(np.full(k, 2.0))
    theta = rng.dirichlet(np.full(k, 2.0))
    for j in range(0, k, 2):                                # pi * theta of a pair: equal, or one to three ulp apart
        theta[j + 1] = theta[j]
        p = pi[j]
        for _ in range(int(rng.randint(0, 4))):
            p = np.nextafter(p, 1.0)
        pi[j + 1] = p
    return raw, pi, theta


# the seeds and keywords tests/test_gpu_round6.py runs near_tie_matrix with
NEAR_TIE_CASES = [(1, {}), (2, dict(max_len=8)), (3, dict(long_rows=40, n=3000)), (4, dict(scores=(1, 2), k=64, max_len=60)),
                  (5, dict(max_len=250, n=1500, k=600))]


def z_value_threshold(ref):
    """a conf threshold that IS a z value of the oracle: the median of the rows' largest z above 0.5 (as tests/test_gpu_round6.py
    picks it); `ref` a Reference of a matrix without empty rows"""
    zmax = np.maximum.reduceat(ref.zn, ref.indptr[:-1])
    big = np.sort(zmax[zmax > 0.5])
    return float(big[len(big) // 2])


def user_z_of(raw, lut, pi, theta, seed=5, drop=0.1):
    """a caller's z for `raw`: the reference's fp64 z of (pi, theta), NaN (no entry) outside its pattern and on a random tenth of
    the entries — not renormalised: the device uses it as it is"""
    zn = numpy_z(oracle_model(raw, lut), raw, pi, theta)
    _, inpat = exact_numerators(raw.indptr, raw.indices, raw.data, lut, pi, theta)
    rng = np.random.RandomState(seed)
    return np.where(inpat & (rng.random_sample(raw.nnz) >= drop), zn, np.nan)


# ---- planted thresholds (leg b) ---------------------------------------------------------------------------------------------------
def planted_values():
    """Every z worth planting, sorted, unique: each entry of phred_table() and its neighbours at +-1 and +-2 ulp, every
    (k + 0.5) / 100 as numpy rounds it and its neighbours, 0.2, 0.9, the exact XP ties 0.125 / 0.375 / 0.625 / 0.875 (and their
    neighbours), 0, 1 and nextafter(1, 0)."""
    from telescope_amd import bam_out
    one = int(np.float64(1.0).view(np.uint64))
    base = np.concatenate([bam_out.phred_table(), (np.arange(100) + 0.5) / 100, [0.2, 0.9, 0.125, 0.375, 0.625, 0.875]])
    bits = base.view(np.uint64).astype(np.int64)
    near = np.concatenate([bits + d for d in range(-2, 3)])
    near = near[(near >= 0) & (near <= one)].astype(np.uint64).view(np.float64)
    return np.unique(np.concatenate([near, [0.0, 1.0, np.nextafter(1.0, 0.0)]]))


def planted_case(table_len, part=0, parts=1):
    """(raw, lut, x): two-entry rows (x, fl(1 - x)) over a caller-supplied ascending score table, kept only where
    x + fl(1 - x) == 1.0 in fp64 — the row sum is then exactly 1, 1 / S and n * r are exact, and the initial z IS x and fl(1 - x),
    bit for bit, in any correct arithmetic.  The table is padded with ascending values above 1 up to `table_len` entries (<= 2048:
    it is staged in LDS in front of the PHRED table; above: it stays in global memory), and the planted values sit at its END when
    it is long, so that a clamped code reads something else.  x[i] is row i's first value.  `part` of `parts`: every parts-th planted
    value (all of them and their complements do not fit 2048 entries)."""
    x = planted_values()[part::parts]
    y = 1.0 - x
    keep = (x + y) == 1.0
    x, y = x[keep], y[keep]
    vals = np.unique(np.concatenate([x, y]))                        # ascending, all in [0, 1]
    assert len(vals) < table_len <= 65536
    pad = table_len - len(vals)
    if table_len <= 2048:
        lut = np.concatenate([vals, 2.0 + np.arange(pad)])
        off = 0
    else:
        lut = np.concatenate([-1.0 - np.arange(pad)[::-1], vals])   # ascending; never referenced by a stored score
        off = pad
    cx = (np.searchsorted(vals, x) + off).astype(np.uint16)
    cy = (np.searchsorted(vals, y) + off).astype(np.uint16)
    n = len(x)
    indptr = 2 * np.arange(n + 1, dtype=np.int64)
    # columns: a pair (2c, 2c + 1) per row, cycling over 64 pairs
    c0 = (2 * (np.arange(n) % 64)).astype(np.int32)
    indices = np.stack([c0, c0 + 1], axis=1).ravel()
    data = np.stack([cx, cy], axis=1).ravel()
    raw = sp.csr_matrix((data, indices, indptr), shape=(n, 128))
    return raw, lut, x


def dyadic_parameters(k, rng):
    """pi and theta that are powers of two, equal within a column pair (2c, 2c + 1): products are exact, and a planted row's
    numerators are (x, fl(1 - x)) times ONE power of two — sums, reciprocal and quotients stay exact."""
    e = rng.randint(-12, -2, k // 2)
    f = rng.randint(-12, -2, k // 2)
    return np.repeat(2.0 ** e, 2), np.repeat(2.0 ** f, 2)
