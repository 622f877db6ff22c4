"""A plain reference of ONE EM pass, ONE log-likelihood pass and ONE parameter update (k_em_fused<P, MODE, FMT, GEO> of
telescope_amd/csrc/tsem_fused.h and the ladder below it, k_colreduce and k_update of tsem_em.hip), the rounding bounds both are held
to, and the seeded matrices and parameter sets that tests/test_em_pass_reference.py (CPU: this reference against the oracle) and
tests/test_gpu_em_pass_exact.py (GPU: the HIP kernels against this reference) share.

numpy and np.longdouble only; the numerators, the row ids, U, TINY and the subnormal convention come from tests/_rowpass_reference.py.
Nothing here touches the engine, so the reference owes nothing to the kernels.

Every bound below is a first-order count of the roundings of the code path it is used for, written next to the count, in the form of
_rowpass_reference.bound and _csr_reference.sum_bound.  None of them was tuned on a kernel's output.
"""
import numpy as np
import scipy.sparse as sp

import _rowpass_reference as R

LD = R.LD
U = R.U
TINY = R.TINY
ABS_SLACK = R.ABS_SLACK
LNL_TERM = 1e-15                                  # every log1p form is within 1e-15 max(1, |log1p|) of libm's
REPRO_CLAIM = 2.0 ** -41                          # include/telescope_em.h, option "reproducible"
REPRO_FLOOR = 2.0 ** -964                         # ... and what a contribution may lose where the grids stop (same sentence)
TWIN_RULE = 1e-12                                 # k_update: twins share one sum while theirs agree to 1e-12
FAIR_RATIO = 2.0 ** 1000


def _sum_by(keys, vals, n):
    """sum of long double `vals` per key in [0, n) (np.bincount has no long double weights): a stable sort and np.add.reduceat"""
    out = np.zeros(n, dtype=LD)
    if len(keys) == 0:
        return out
    order = np.argsort(keys, kind='stable')
    k = np.asarray(keys)[order]
    first = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
    out[k[first]] = np.add.reduceat(np.asarray(vals, dtype=LD)[order], first)
    return out


def _max_by(keys, vals, n):
    out = np.zeros(n, dtype=np.int64)
    if len(keys):
        np.maximum.at(out, keys, vals)
    return out


class RowState(object):
    """What the three references share for one (matrix, parameters): long double numerators n (Q pi theta on rows of several stored
    entries, Q pi on single-entry rows: model.py:699-714), the pattern, row sums S, the rows that are live (recip0: a sum of 0, or
    one so small that fp64's 1 / S is inf, gives z = 0 on the whole row: sparse_plus.py:16-22), w_i = max_j Q_ij and z = n / S."""

    def __init__(self, indptr, indices, raw, lut, pi, theta):
        self.indptr = ip = np.asarray(indptr, dtype=np.int64)
        self.indices = np.asarray(indices)
        self.lens = np.diff(ip)
        self.rid = R.row_ids(ip)
        self.q64 = np.asarray(lut, dtype=np.float64)[np.asarray(raw)]
        n, inpat = R.exact_numerators(ip, indices, raw, lut, pi, theta)
        self.n = np.where(inpat, n, LD(0))
        self.inpat = inpat
        c64 = np.asarray(pi, dtype=np.float64) * np.asarray(theta, dtype=np.float64)
        with np.errstate(under='ignore'):
            n64 = self.q64 * c64[self.indices]
        self.gradual = inpat & ((np.abs(c64) < TINY)[self.indices] | (np.abs(n64) < TINY))     # products on the subnormal grid
        self.S = R._row_reduce(np.add, self.n, ip, LD(0))
        with np.errstate(divide='ignore', over='ignore'):
            self.live = np.isfinite(1.0 / self.S.astype(np.float64))
        self.w = R._row_reduce(np.maximum, self.q64, ip, 0.0)
        self.amb = self.lens > 1
        z = np.zeros(len(self.n), dtype=LD)
        ok = self.live[self.rid]
        z[ok] = self.n[ok] / self.S[self.rid][ok]
        self.z = z


def exact_colsums(indptr, indices, raw, lut, pi, theta, state=None):
    """(sums, cnt, lenmax, gradual): what tsem_em_pass leaves in red[0..K).  sums[j] = sum over the rows of several stored entries of
    w_i z_ij, w_i = max_j Q_ij, z_ij = n_ij / sum_j n_ij, n_ij = Q_ij pi_j theta_j, z = 0 on a row whose sum is 0 (recip0), in long
    double (its own error: about (len + cnt) 2^-64, 2^-11 of the bounds).  cnt[j]: the entries that contribute to column j (non-zero
    numerator, live row); lenmax[j]: the most stored entries of a row that contributes to it; gradual[j]: the sum over j's
    contributing entries whose pi theta or Q pi theta is subnormal of one step of the subnormal grid times s_i = w_i / S_i — gradual
    underflow is no relative rounding (see ABS_SLACK of _rowpass_reference): such a numerator carries an absolute error of up to
    2^-1075 whichever way it is formed (Q c rounded onto the grid, or c alone where a layout multiplies by c last), and the scatter
    multiplies it by s_i."""
    st = state or RowState(indptr, indices, raw, lut, pi, theta)
    k = len(pi)
    use = st.amb[st.rid] & st.live[st.rid] & st.inpat & (st.n != 0)
    s = np.zeros(len(st.lens), dtype=LD)
    ok = st.amb & st.live
    s[ok] = st.w[ok].astype(LD) / st.S[ok]
    cols = st.indices[use]
    sums = _sum_by(cols, (st.z * st.w.astype(LD)[st.rid])[use], k)
    cnt = np.bincount(cols, minlength=k).astype(np.int64)
    lenmax = _max_by(cols, st.lens[st.rid][use], k)
    g = use & st.gradual
    gradual = _sum_by(st.indices[g], s[st.rid][g] * LD(ABS_SLACK), k)
    return sums, cnt, lenmax, gradual


def oracle_slack(state, k):
    """The reference's operator sequence forms z = n fl(1 / S) BEFORE it multiplies by w: a z below 2^-1022 lands on the subnormal
    grid (or on 0) there, an absolute error of up to one step, times w_i.  Per column, the sum of w_i 2^-1074 over its contributing
    entries with such a z.  The kernels form s = w fl(1 / S) first and do not need it."""
    st = state
    small = st.amb[st.rid] & st.live[st.rid] & (st.z > 0) & (st.z < LD(TINY))
    return _sum_by(st.indices[small], st.w.astype(LD)[st.rid][small] * LD(ABS_SLACK), k)


# ---- bounds of the column sums ----------------------------------------------------------------------------------------------------
FUSED, SPLIT, UNTAGGED, ORACLE = 'fused', 'split', 'untagged', 'oracle'


def colsum_bound(cnt, lenmax, path=FUSED, P=1):
    """Relative bound of one column sum, first order, in units of 2^-53, as a function of counts.

    A term w_i z_ij of the fused kernel is n s with n = fl(Q fl(pi theta)) (two roundings), s = fl(w fl(1 / S)) (two) and the
    product (one): 5.  S is a sum of len positive terms: len - 1 for ANY order of the additions, the members' partial sums
    included.  With P > 1 members every member's partial row sum crosses the exchange with its mantissa LSB overwritten by the
    epoch tag: at most one ulp = 2 x 2^-53 per member, 2 P.  The column adds cnt positive terms through LDS accumulators, hot-column
    copies, team partials and k_colreduce: cnt - 1 for any order.  Together (lenmax + cnt + 2 P + 3) 2^-53: c0 = 5 - 1 - 1.
      FUSED     c0 = 3, tags 2 P (P = 1: no exchange, no tag: the term is dropped)
      SPLIT     the scatter adds Q s and k_colreduce multiplies the sum by cmul = pi theta: the same five roundings in another order
                (pi theta, 1 / S, w r, Q s, cmul t) — and one more, the split row-sum pass forms Q c a second time for S: c0 = 4;
                its members' partial row sums travel untagged through HBM (k_row_factors): no tag term
      UNTAGGED  the two-pass kernels and the CSR row passes (k_em_rows): the five roundings, no tag: c0 = 3
      ORACLE    scipy's fp64 operator sequence (estep -> z.multiply(weights).multiply(Y).sum(0)): z = n fl(1 / S) and z w are
                the same five roundings: c0 = 3, no tag
    A column without contributing entries has the bound 0: its sum is exactly 0 on both sides."""
    cnt = np.asarray(cnt).astype(LD)
    c0 = {FUSED: 3, SPLIT: 4, UNTAGGED: 3, ORACLE: 3}[path]
    tags = 2 * P if (path == FUSED and P > 1) else 0
    return np.where(cnt > 0, (np.asarray(lenmax).astype(LD) + cnt + tags + c0) * LD(U), LD(0))


def repro_bound(cnt, lenmax, P=1):
    """Option "reproducible", relative.  include/telescope_em.h documents the column sums as "within (entries of the column) x 2^-41
    of exact": that is the ACCUMULATION — every contribution v = n s is cut on the column's grid 2^E into a multiple of 2^(E-30), a
    multiple of 2^(E-60) and a remainder of at most 2^(E-61) that is dropped, and the sums of the pieces are exact — stated relative
    to the sum S, because k_bin_check accepts a grid only while E is at most BIN_SLACK + 4 = 20 bits above S's exponent: cnt dropped
    remainders are at most cnt 2^(E-61) <= cnt 2^-41 S.  That term takes the place of the cnt - 1 additions of colsum_bound; the
    contributions themselves are formed as in the default mode ((lenmax + 2 P + 4) 2^-53, see colsum_bound: five roundings, len - 1
    additions, the tags), and S = high + low is one more rounding.  The grids stop at 2^-903 (k_bin_check lowers an empty column's
    no further than ebias 120), where the dropped remainder is at most 2^(-903 - 61): repro_limit adds cnt 2^-964 absolute."""
    cnt = np.asarray(cnt).astype(LD)
    tags = 2 * P if P > 1 else 0
    return np.where(cnt > 0, (np.asarray(lenmax).astype(LD) + tags + 5) * LD(U) + cnt * LD(REPRO_CLAIM), LD(0))


def repro_limit(ref, P):
    """the absolute limits of a PassReference's column sums under option `reproducible`"""
    return repro_bound(ref.cnt, ref.lenmax, P) * ref.sums + ref.gradual + ref.cnt.astype(LD) * LD(max(ABS_SLACK, REPRO_FLOOR))


def colsum_fraction(red, sums, cnt, lenmax, gradual, path=FUSED, P=1, limit=None):
    """(largest |red - sums| / limit, its column): limit_j = bound_j sums_j + gradual_j + cnt_j 2^-1074 (a subnormal product n s is
    given one step of the grid), or the caller's absolute `limit`.  inf where the limit is 0 and the value differs: a zero is
    exact."""
    red = np.asarray(red, dtype=np.float64)
    if limit is None:
        limit = colsum_bound(cnt, lenmax, path, P) * np.abs(sums) + gradual + np.asarray(cnt).astype(LD) * LD(ABS_SLACK)
    err = np.abs(red.astype(LD) - sums)
    frac = np.zeros(len(err), dtype=np.float64)
    ok = limit > 0
    frac[ok] = (err[ok] / limit[ok]).astype(np.float64)
    frac[~ok & (err > 0)] = np.inf
    frac[np.isnan(red)] = np.inf
    j = int(np.argmax(frac)) if len(frac) else 0
    return (float(frac[j]) if len(frac) else 0.0), j


# ---- log-likelihood ---------------------------------------------------------------------------------------------------------------
def exact_lnl(indptr, indices, raw, lut, pi_prev, theta_prev, pi, theta, P=0, prev_state=None):
    """(lnl, limit, info): sum over ALL rows, single-entry rows included, of z(prev)_ij log1p(n(cur)_ij), as
    OracleModel.calculate_lnl (model.py:744-760) with z of the previous parameters; np.log1p on long doubles.

    limit, absolute: per term, z's relative bound times |term| — z = n fl(1 / S): (len + 3) 2^-53 as _rowpass_reference.bound, plus
    2 P for the tag bits of a fused layout's partial row sums (P > 1), plus one rounding for the product z l —; the argument of
    log1p carries two roundings (pi theta, Q c) and d log1p(x) = dx / (1 + x), at most 2 x 2^-53 min(x, 1) <= 2 x 2^-53 absolute,
    times z; the logarithm itself 1e-15 max(1, |log1p|) times z; and (terms) 2^-53 sum|term| for any order of adding
    them.  info: sum|term|, sum z max(1, |log1p|), the number of terms."""
    st = prev_state or RowState(indptr, indices, raw, lut, pi_prev, theta_prev)
    n, inpat = R.exact_numerators(st.indptr, indices, raw, lut, pi, theta)
    with np.errstate(over='ignore'):
        l = np.log1p(np.where(inpat, n, LD(0)))
    term = st.z * l
    mag = np.maximum(LD(1), np.abs(l))
    tags = 2 * P if P > 1 else 0
    zrel = (st.lens[st.rid].astype(LD) + 4 + tags) * LD(U)
    nterm = int(np.count_nonzero(term))
    sum_abs = np.abs(term).sum()
    zmag = (st.z * mag).sum()
    limit = (zrel * np.abs(term)).sum() + 2 * LD(U) * st.z.sum() + LD(LNL_TERM) * zmag + nterm * LD(U) * sum_abs
    return term.sum(), limit, dict(sum_abs=sum_abs, zmag=zmag, terms=nterm)


# ---- update -----------------------------------------------------------------------------------------------------------------------
def twin_representatives(col_count, col_hash):
    """rep[j]: the smallest column with j's (count, signature) of tsem_rowstats — columns with the same fragments and scores; a
    column without entries stands for itself (tsem_set_model)."""
    cnt = np.asarray(col_count, dtype=np.uint64)
    hsh = np.asarray(col_hash, dtype=np.uint64)
    k = len(cnt)
    order = np.lexsort((np.arange(k), hsh, cnt))
    first = np.concatenate([[True], (cnt[order][1:] != cnt[order][:-1]) | (hsh[order][1:] != hsh[order][:-1])])
    rep = np.empty(k, dtype=np.int64)
    rep[order] = order[np.maximum.accumulate(np.where(first, np.arange(k), 0))]
    rep[cnt == 0] = np.flatnonzero(cnt == 0)
    return rep


def twin_rule(v, rep):
    """k_update / tsem_set_model: a twin takes its representative's sum where the two agree to 1e-12 relative, its own otherwise."""
    v = np.asarray(v, dtype=np.float64)
    r = v[rep]
    take = np.abs(v - r) <= TWIN_RULE * np.maximum(np.abs(v), np.abs(r))
    return np.where(take, r, v), take


def exact_update(red, pisum0, stats, priors, pi_old, K=None):
    """(pi_hat, theta_hat, diff) — the closed forms of mstep (model.py:733-740) in fp64, every operation correctly rounded and in
    the order of the reference: theta_hat = (thetasum + theta_prior_wt) / (ambig_wt + theta_prior_wt K); pisum = pisum0 +
    thetasum; pi_hat = (pisum + pi_prior_wt) / (total_wt + pi_prior_wt K), prior weights = prior x the largest weight (model.py:
    696-697) — and diff_est = sum |pi_hat - pi| (model.py:781) of those fp64 values in long double.  `red`: the column sums as they
    are (twins already merged by the caller where the rule applies); stats = (total_wt, ambig_wt, largest weight)."""
    red = np.asarray(red, dtype=np.float64)
    K = len(red) if K is None else K
    w_tot, w_amb, w_max = (float(x) for x in stats)
    pi_prior, theta_prior = priors
    tpw, ppw = np.float64(theta_prior) * np.float64(w_max), np.float64(pi_prior) * np.float64(w_max)
    tden, pden = np.float64(w_amb) + tpw * np.float64(K), np.float64(w_tot) + ppw * np.float64(K)
    with np.errstate(divide='ignore', invalid='ignore'):
        theta_hat = (red + tpw) / tden
        pi_hat = ((np.asarray(pisum0, dtype=np.float64) + red) + ppw) / pden
    diff = np.abs(pi_hat.astype(LD) - np.asarray(pi_old, dtype=np.float64).astype(LD)).sum()
    return pi_hat, theta_hat, diff


def diff_bound(K, diff):
    """diff_est adds K non-negative terms |pi_hat - pi|, each one rounding, in any order: K 2^-53 sum|pi_hat - pi|."""
    return LD(K) * LD(U) * diff


# ---- fairness ---------------------------------------------------------------------------------------------------------------------
def fair(indptr, indices, raw, lut, pi, theta, state=None):
    """The reasons, if any, why (matrix, parameters) is no fair input of a comparison at rounding level; [] = fair.  Taken from the
    reference's own numbers, before any device value is looked at.
      * a row of several entries with w_i / S_i >= 2^1000: the device forms s = w (1 / S) before it multiplies by n, the reference
        n (1 / S) first, and s overflows where z does not.  Such a row needs EVERY one of its columns below about 1e-285 — an M-step
        cannot produce that: theta_hat >= theta_prior_wt / theta_den, and with theta_prior = 0 a column with sum 0 is exactly 0 and
        leaves the pattern instead;
      * a row sum in (0, 2^-1020): whether 1 / S is inf (recip0: the row is dropped) then hangs on the order the row was added in;
      * a NaN, an inf or a negative parameter."""
    st = state or RowState(indptr, indices, raw, lut, pi, theta)
    why = []
    for name, v in (('pi', pi), ('theta', theta)):
        v = np.asarray(v, dtype=np.float64)
        if not np.all(np.isfinite(v)) or np.any(v < 0):
            why.append('%s is not finite and non-negative' % name)
    low = (st.S > 0) & (st.S < LD(2.0) ** -1020)
    if low.any():
        why.append('%d rows with a sum in (0, 2^-1020): recip0 hangs on the order of additions' % int(low.sum()))
    ok = st.amb & st.live & (st.S > 0)
    big = ok.copy()
    big[ok] = st.w[ok].astype(LD) / st.S[ok] >= LD(FAIR_RATIO)
    if big.any():
        why.append('%d rows with w / S >= 2^1000 (first: row %d)' % (int(big.sum()), int(np.flatnonzero(big)[0])))
    return why


def fair_stops(values, epsilon, rel=1e-6):
    """For integer-valued comparisons (iteration counts under em_chunk): the stop tests `value < epsilon` that lie within `rel` of
    epsilon — rounding could decide them either way (as tests/test_gpu_bootstrap.py does); [] = fair."""
    v = np.asarray(values, dtype=np.float64)
    if epsilon == 0.0:
        return []
    return [int(i) for i in np.flatnonzero(np.abs(v - epsilon) <= rel * abs(epsilon))]


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
MAX_SCORE = 212                                  # the reference's table: Q = expm1(100 r / 212), e^0.47 - 1 ... e^100 - 1


def lut(raw=None):
    """the model's own score table for `raw` (its largest score; MAX_SCORE for every matrix built here, the synthetic zipf matrix
    brings its own)"""
    from telescope_amd.likelihood import score_lut
    return score_lut(MAX_SCORE if raw is None else int(raw.data.max()))


def _coo_csr(rows, cols, data, shape):
    m = sp.csr_matrix((np.asarray(data, dtype=np.uint16), (np.asarray(rows), np.asarray(cols))), shape=shape)
    m.sort_indices()
    assert m.data.min(initial=1) >= 1, 'a stored score of 0 (or two entries in one cell)'
    return m


def ring_matrix(n_rows, k, seed=1, lo=2, hi=12, min_score=1):
    """`n_rows` rows of lo .. hi entries over k columns, all ambiguous but for 5 % single-entry rows: many blocks of short rows, so
    that every team of the fused kernel walks its register ring (FZ_NS sets) and its exchange ring (FZ_XS slots) round more than
    twice.  Scores from the whole table (Q over 43 decades) unless min_score says otherwise."""
    rng = np.random.RandomState(R._seed('ring', n_rows, k, seed))
    lens = rng.randint(lo, hi + 1, n_rows)
    lens[rng.random_sample(n_rows) < 0.05] = 1
    lens[0] = lens[-1] = hi
    m = R.matrix_from_lengths(lens, k, MAX_SCORE, rng, tie_scores=0.1)
    if min_score > 1:
        m.data = np.maximum(m.data, min_score).astype(np.uint16)
    return m


def short_row_matrix(n_rows, k, seed=2):
    """rows of 2 - 6 entries (geometry 3 of the fused kernel)"""
    return ring_matrix(n_rows, k, seed=seed, lo=2, hi=6)


def zipf_matrix(n_rows, k, mean=12.0, seed=3):
    """zipf-distributed columns (a few columns hold a large share of the entries: hot columns), a tenth single-entry rows"""
    from telescope_amd import synthetic
    m = synthetic.generate_csr(n_rows, k, mean, seed=seed, dist='zipf', uniq_frac=0.1)
    m.sort_indices()
    return m


ROW_SHAPE_LENGTHS = (2, 3, 4, 5, 8, 9, 63, 64, 65, 255, 256, 257, 1000)


def row_shape_matrix(k=6000, filler=2400, reps=3, seed=4):
    """Rows of every length at which a kernel changes its path — ROW_SHAPE_LENGTHS `reps` times each, and one row that holds every
    column an ambiguous row may hold (k - 2 entries) — among `filler` rows of 2 - 40 entries; a fifth single-entry rows; two empty
    rows; the first and the last row ambiguous.  Special columns:
      0 / 1        exact twins and hot: column 0 sits in 40 % of the filler rows, column 1 in the same rows with the same scores
      S2 / k - 3   exact twins, ordinary: column k - 3 is a copy of column S2 = 7
      k - 2        occurs in single-entry rows only
      k - 1        occurs nowhere
    Returns (raw, special) with special = dict(hot=(0, 1), twin=(7, k - 3), unique_only=k - 2, nowhere=k - 1)."""
    rng = np.random.RandomState(R._seed('rowshape', k, filler, reps, seed))
    S2, T2, UNQ, NOW = 7, k - 3, k - 2, k - 1
    general = np.setdiff1d(np.arange(k), [0, 1, T2, UNQ, NOW])                      # ascending: a remap keeps rows sorted
    edge_cols = np.setdiff1d(general, [S2])                                         # the rows of an exact length hold no twin source
    edge = np.array(ROW_SHAPE_LENGTHS * reps)
    fill = rng.randint(2, 41, filler)
    fill[rng.random_sample(filler) < 0.2] = 1
    e = R.matrix_from_lengths(edge, len(edge_cols), MAX_SCORE, rng, tie_scores=0.1).tocoo()
    f = R.matrix_from_lengths(fill, len(general), MAX_SCORE, rng, tie_scores=0.1).tocoo()
    # row order: [a filler row] [edge and filler rows shuffled, two empty rows among them] [the full row] [a filler row]
    n_mid = len(edge) + filler - 2 + 2
    perm = rng.permutation(n_mid) + 1
    e_row = perm[:len(edge)]
    f_ids = np.flatnonzero(fill > 1)[:2]                                            # two ambiguous filler rows go first and last
    rest = np.setdiff1d(np.arange(filler), f_ids)
    f_row = np.empty(filler, dtype=np.int64)
    f_row[rest] = perm[len(edge):len(edge) + len(rest)]
    n_rows = n_mid + 3
    f_row[f_ids[0]], f_row[f_ids[1]] = 0, n_rows - 1
    full_row = n_rows - 2
    rows = [e_row[e.row], f_row[f.row]]
    cols = [edge_cols[e.col], general[f.col]]
    data = [e.data, f.data]
    # the full row: every general column and column 0
    rows.append(np.full(len(general) + 1, full_row)); cols.append(np.concatenate([[0], general]))
    data.append(rng.randint(1, MAX_SCORE + 1, len(general) + 1))
    # column 0 in 40 % of the ambiguous filler rows
    hot_rows = f_row[(fill > 1) & (rng.random_sample(filler) < 0.4)]
    rows.append(hot_rows); cols.append(np.zeros(len(hot_rows), dtype=np.int64)); data.append(rng.randint(1, MAX_SCORE + 1, len(hot_rows)))
    rows, cols, data = np.concatenate(rows), np.concatenate(cols), np.concatenate(data)
    # some single-entry rows move to the column that only such rows hold
    single = f_row[fill == 1]
    move = np.isin(rows, single[::7])
    cols = np.where(move, UNQ, cols)
    # the twins: column 1 copies column 0, column k - 3 copies column S2 (single-entry rows of S2 become two-entry rows: still twins)
    for src, dst in ((0, 1), (S2, T2)):
        sel = cols == src
        rows, cols, data = np.concatenate([rows, rows[sel]]), np.concatenate([cols, np.full(sel.sum(), dst)]), np.concatenate([data, data[sel]])
    raw = _coo_csr(rows, cols, data, (n_rows, k))
    lens = np.diff(raw.indptr)
    assert lens[0] > 1 and lens[-1] > 1 and (lens == 0).sum() == 2 and lens.max() == k - 2
    assert all((lens == l).sum() >= reps for l in ROW_SHAPE_LENGTHS), 'an edge length is missing'
    csc = raw.tocsc()
    assert csc[:, NOW].nnz == 0 and csc[:, UNQ].nnz > 0 and np.all(lens[csc[:, UNQ].indices] == 1)
    for a, b in ((0, 1), (S2, T2)):
        assert csc[:, a].nnz > 0 and (csc[:, a] != csc[:, b]).nnz == 0
    return raw, dict(hot=(0, 1), twin=(S2, T2), unique_only=UNQ, nowhere=NOW)


def wide_matrix(k, n_rows=3000, seed=5):
    """a few thousand rows of 2 - 40 entries over very many columns (the upper rungs of the K ladder), a tenth single-entry rows"""
    rng = np.random.RandomState(R._seed('wide', k, n_rows, seed))
    lens = rng.randint(2, 41, n_rows)
    lens[rng.random_sample(n_rows) < 0.1] = 1
    lens[0] = lens[-1] = 9
    return R.matrix_from_lengths(lens, k, MAX_SCORE, rng, tie_scores=0.1)


# ---- parameter sets ---------------------------------------------------------------------------------------------------------------
PARAMETER_SETS = ('uniform', 'decades', 'dying', 'dead_rows', 'subnormal', 'lnl_straddle_sparse', 'lnl_straddle_dense')
FLOOR = 1e-12                                     # `dying`: every ambiguous row keeps a column with pi theta >= FLOOR / K


def _normalised(v):
    s = v.sum()
    return v / s if s > 0 and np.isfinite(s) else v


def _rescue(raw, weak, rng):
    """One column per ambiguous row (a random stored one) is marked as not weak, until every ambiguous row holds one."""
    weak = weak.copy()
    lens = np.diff(raw.indptr)
    amb = np.flatnonzero(lens > 1)
    pick = raw.indptr[amb] + (rng.random_sample(len(amb)) * lens[amb]).astype(np.int64)
    strong_per_row = np.add.reduceat((~weak)[raw.indices].astype(np.int64), raw.indptr[:-1][lens > 0])
    has = np.zeros(len(lens), dtype=bool)
    has[lens > 0] = strong_per_row > 0
    need = ~has[amb]
    weak[raw.indices[pick[need]]] = False
    return weak


def parameter_set(name, raw, seed=0):
    """(pi, theta) of PARAMETER_SETS[name] for the matrix `raw`, seeded; each vector sums to 1 up to rounding where that is possible.
      uniform     pi = theta = 1 / K
      decades     log-uniform over 12 decades in pi and, independently, in theta
      dying       a third of the columns with pi in 1e-300 .. 1e-20, a further 2 % exactly 0 in pi and 2 % exactly 0 in theta;
                  every ambiguous row keeps a column with pi theta >= 1e-12 / K (constructed so, and asserted)
      dead_rows   `dying`, and about 1 % of the ambiguous rows with EVERY column exactly 0 (recip0(0))
      subnormal   `decades`, and a few columns whose pi theta is below 2^-1022 but above 0
      lnl_straddle_sparse / _dense
                  pi theta spread so that Q pi theta of the stored scores falls above 2^27, below e^-40 and between the two in one
                  pass: most columns far above 2^27 for every stored score; a share of 1e-4 (sparse: below the device's 0.1 %
                  selection limit of the log-table form) or 20 % (dense: above it) of the columns placed inside the window."""
    k = raw.shape[1]
    rng = np.random.RandomState(R._seed('params', name, k, raw.nnz, seed))
    if name == 'uniform':
        return np.full(k, 1.0 / k), np.full(k, 1.0 / k)
    pi = _normalised(10.0 ** rng.uniform(-12, 0, k))
    theta = _normalised(10.0 ** rng.uniform(-12, 0, k))
    if name == 'decades':
        return pi, theta
    if name == 'subnormal':
        few = np.flatnonzero(_rescue(raw, np.isin(np.arange(k), rng.choice(k, max(3, k // 500), replace=False)), rng))
        pi[few] = 10.0 ** rng.uniform(-160, -155, len(few))
        theta[few] = 10.0 ** rng.uniform(-158, -155, len(few))
        c = pi[few] * theta[few]
        pi, theta = _normalised(pi), _normalised(theta)
        c = pi[few] * theta[few]
        assert len(few) > 0 and np.all(c > 0) and np.all(c < TINY)
        return pi, theta
    if name in ('dying', 'dead_rows'):
        pi = _normalised(10.0 ** rng.uniform(-3, 0, k))
        theta = _normalised(10.0 ** rng.uniform(-3, 0, k))
        u = rng.random_sample(k)
        weak = _rescue(raw, u < 1 / 3 + 0.04, rng)
        dying = weak & (u < 1 / 3)
        pi[dying] = 10.0 ** rng.uniform(-300, -20, int(dying.sum()))
        pi[weak & (u >= 1 / 3) & (u < 1 / 3 + 0.02)] = 0.0
        theta[weak & (u >= 1 / 3 + 0.02)] = 0.0
        pi, theta = _normalised(pi), _normalised(theta)
        lens = np.diff(raw.indptr)
        best = np.maximum.reduceat((pi * theta)[raw.indices], raw.indptr[:-1][lens > 0])
        assert np.all(best[lens[lens > 0] > 1] >= FLOOR / k), 'an ambiguous row without a column of pi theta >= 1e-12 / K'
        if name == 'dead_rows':
            # about 1 % of the ambiguous rows, the shortest first — or as many as a tenth of the columns make: a dead row takes all its
            # columns with it, in every other row too (rows that lose their last live column this way are dead rows as well)
            amb = np.flatnonzero(lens > 1)
            amb = amb[np.argsort(lens[amb] + rng.random_sample(len(amb)), kind='stable')]
            dead = amb[:max(2, min(len(amb) // 100, k // (10 * max(2, int(lens[amb[0]])))))]
            rid = R.row_ids(raw.indptr)
            pi[raw.indices[np.isin(rid, dead)]] = 0.0
            full = lens > 0
            for _ in range(50):                                     # a row left with dying columns only dies as a whole
                c = (pi * theta)[raw.indices]
                strong = np.maximum.reduceat(c, raw.indptr[:-1][full]) >= 2 * FLOOR / k
                alive = np.maximum.reduceat(c, raw.indptr[:-1][full]) > 0
                bad = np.zeros(len(lens), dtype=bool)
                bad[full] = alive & ~strong
                bad &= lens > 1
                if not bad.any():
                    break
                pi[raw.indices[bad[rid]]] = 0.0
            assert not bad.any()
            pi = _normalised(pi)
        return pi, theta
    if name.startswith('lnl_straddle'):
        # for a matrix whose stored scores are 139 .. 212: log Q in [65.5, 100].  Columns outside the window: pi theta about 1 / K,
        # log Q + log c > 50: far above 18.7 (2^27) for every stored score.  Window columns: log c = -125 gives log Q + log c in
        # [-59.5, -25] (below e^-40 and between), log c = -70 gives [-4.5, 30] (between and above).  sparse: exactly these two columns,
        # of median popularity (well below the device's selection limit of 0.1 % of the stored entries once K >= 4000); dense: a fifth
        # of the columns, log c uniform in [-140, -60].
        pi = _normalised(10.0 ** rng.uniform(-1, 0, k))
        theta = np.full(k, 1.0 / k)
        if name.endswith('sparse'):
            cnt = np.bincount(raw.indices, minlength=k)
            two = np.argsort(np.abs(cnt - np.median(cnt)), kind='stable')[:2]
            theta[two] = np.exp([-125.0, -70.0]) / pi[two]
        else:
            inside = _rescue(raw, rng.random_sample(k) < 0.2, rng)
            theta[inside] = np.exp(rng.uniform(-140, -60, int(inside.sum()))) / pi[inside]
        return pi, _normalised(theta)
    raise KeyError(name)


def straddle_counts(raw, lut_, pi, theta):
    """how many stored entries of ambiguous rows have Q pi theta >= 2^27, in [e^-40, 2^27) and in (0, e^-40)"""
    lens = np.diff(raw.indptr)
    amb = (lens > 1)[R.row_ids(raw.indptr)]
    with np.errstate(under='ignore'):
        x = (np.asarray(lut_)[raw.data] * (pi * theta)[raw.indices])[amb]
    return int((x >= 2.0 ** 27).sum()), int(((x >= np.exp(-40.0)) & (x < 2.0 ** 27)).sum()), int(((x > 0) & (x < np.exp(-40.0))).sum())


# ---- the oracle's fp64 results (CPU file) -----------------------------------------------------------------------------------------
def oracle_pass(raw, lut_, pi, theta, pi_prev=None, theta_prev=None):
    """(column sums, lnl) of the reference's fp64 operator sequence: estep -> z.multiply(weights).multiply(Y).sum(0) and
    calculate_lnl(z(prev), cur) on an OracleModel whose Q is lut_[raw]."""
    om = R.oracle_model(raw, lut_)
    om.weights = om.Q.max(1)
    with np.errstate(over='ignore', under='ignore', divide='ignore'):
        z = om.estep(np.asarray(pi, dtype=np.float64), np.asarray(theta, dtype=np.float64))
        sums = np.asarray(sp.csr_matrix(z.multiply(om.weights)).multiply(om.Y).sum(0)).ravel()
        zp = z if pi_prev is None else om.estep(np.asarray(pi_prev, dtype=np.float64), np.asarray(theta_prev, dtype=np.float64))
        lnl = float(om.calculate_lnl(zp, np.asarray(pi, dtype=np.float64), np.asarray(theta, dtype=np.float64)))
    return sums, lnl, om


# ---- the cases both files run -----------------------------------------------------------------------------------------------------
MATRICES = ('row_shape', 'row_shape_p1', 'ring', 'ring_hi', 'short', 'zipf', 'wide_70k', 'wide_500k')
REDUCED = {'ring': 3000, 'ring_hi': 3000, 'short': 3000, 'zipf': 3000, 'wide_70k': 400, 'wide_500k': 400}
_cache = {}


def matrix(name, rows=None):
    """The seeded matrix `name` with `rows` rows (None: the size the GPU file uses where it does not compute one; the row-shape
    matrix has one size), cached.
      row_shape  row_shape_matrix()                      ring     2 - 12 entries over 4000 columns, scores 1 .. 212
      row_shape_p1  the same over 3400 columns: its row of K - 2 entries fits ONE register tile of the fused kernel (3584 entries),
                 which a layout of a single column part needs — with 6000 columns that layout falls to the two-pass kernels
      ring_hi    `ring` with scores 139 .. 212 (the lnl_straddle sets are built for it)
      short      2 - 6 entries over 16 000 columns       zipf     zipf columns over 6000, ~12 entries per row
      wide_70k / wide_500k   2 - 40 entries over 70 000 / 500 000 columns"""
    key = (name, rows)
    if key not in _cache:
        if name == 'row_shape':
            m = row_shape_matrix()[0]
        elif name == 'row_shape_p1':
            m = row_shape_matrix(k=3400)[0]
        elif name == 'ring':
            m = ring_matrix(rows or 40000, 4000)
        elif name == 'ring_hi':
            m = ring_matrix(rows or 20000, 4000, seed=6, min_score=139)
        elif name == 'short':
            m = short_row_matrix(rows or 30000, 16000)
        elif name == 'zipf':
            m = zipf_matrix(rows or 30000, 6000)
        elif name in ('wide_70k', 'wide_500k'):
            m = wide_matrix(70000 if name == 'wide_70k' else 500000, rows or 3000)
        else:
            raise KeyError(name)
        _cache[key] = m
    return _cache[key]


class PassReference(object):
    """Everything one (matrix, previous parameters, current parameters) needs: the fairness verdict, the exact column sums of the
    current parameters with their counts, and the exact lnl of z(previous) against the current ones."""

    def __init__(self, raw, lut_, pi, theta, pi_prev=None, theta_prev=None, want_lnl=True):
        a = (raw.indptr, raw.indices, raw.data, lut_)
        self.pi, self.theta = np.asarray(pi, dtype=np.float64), np.asarray(theta, dtype=np.float64)
        self.state = RowState(*a, self.pi, self.theta)
        self.fair = fair(*a, self.pi, self.theta, state=self.state)
        self.sums, self.cnt, self.lenmax, self.gradual = exact_colsums(*a, self.pi, self.theta, state=self.state)
        same = pi_prev is None
        self.prev = self.state if same else RowState(*a, np.asarray(pi_prev, dtype=np.float64), np.asarray(theta_prev, dtype=np.float64))
        if not same:
            self.fair = self.fair + fair(*a, pi_prev, theta_prev, state=self.prev)
        if want_lnl:
            self.lnl, self.lnl_limit, self.lnl_info = exact_lnl(*a, None, None, self.pi, self.theta, P=0, prev_state=self.prev)

    def lnl_limit_P(self, P):
        """the lnl limit for a fused layout of P members: the tag term 2 P 2^-53 sum|term| on top of the untagged limit"""
        return self.lnl_limit + (2 * P if P > 1 else 0) * LD(U) * self.lnl_info['sum_abs']
