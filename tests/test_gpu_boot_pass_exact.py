"""`-m gpu`: the bootstrap unit (telescope_amd/csrc/tsem_boot.hip: k_boot_sweep<0|1|2|3>, k_boot_init, k_boot_update, k_boot_finish,
the fold kernels) after 1, 2 and 3 iterations against tests/_boot_pass_reference.py: an exact (long double) reference of the weighted
closed form with rounding bounds that are functions of counts, tied down without a GPU by tests/test_boot_pass_reference.py.

What every call is checked for, per replicate (`_check`), through _lib.Engine.bootstrap / bootstrap_groups with explicit
multiplicities unless the leg says otherwise:
 1. n_frags, n_iter, converged equal;
 2. pi and theta within their bounds on every column, exact zeros exactly 0, NaN only where the reference has NaN;
 3. lnl within its limit;
 4. the counts of exclude, unique and all equal, those of average and conf within their bounds;
 5. grouped calls: the pattern equal; X_b per slot equal (integer methods) or within bounds; mean and sd equal numpy's Welford in
    replicate order on the device's own kept values bit for bit, and within bounds of the reference's.
Every input is fair by the reference alone (asserted here and, without a device, in the CPU file): no leg skips a row, a column, a
replicate or a method.  The legs print `BOOTPASS ...` lines with the figures they assert on, the largest error as a fraction of its
bound among them (`pytest -s`); profiles/r26_boot_pass_exact.txt keeps a run."""
import numpy as np
import pytest

import _boot_pass_reference as P

pytestmark = pytest.mark.gpu
LD = P.LD
ITERS = (1, 2, 3)
_faulted = []                                     # HIP errors met so far: after one, nothing more is started on the device
_devs = {}


def _say(fmt, *a):
    print('BOOTPASS ' + fmt % a, flush=True)


@pytest.fixture(autouse=True)
def _nothing_after_a_fault():
    if _faulted:
        pytest.fail('an earlier test of this file met a HIP error (%s): no further work is started on the device' % _faulted[0])
    yield


def _engine(gpu_device):
    """an _lib.Engine that remembers a HIP error (TSEM_ERR_HIP, TSEM_ERR_TIMEOUT) for the fixture above"""
    from telescope_amd import _lib

    class Engine(_lib.Engine):
        def _ck(self, rc):
            if rc in (-2, -4):
                _faulted.append('libtelescope_em error %d: %s' % (rc, self._L.tsem_last_error(self._h).decode()))
            _lib.Engine._ck(self, rc)
    return Engine(gpu_device)


@pytest.fixture(scope='module')
def cu_count(gpu_device):
    import torch
    return int(torch.cuda.get_device_properties(gpu_device).multi_processor_count)


OPTION_DEFAULTS = {'boot_rows_per_block': 0, 'boot_hot_columns': -1, 'boot_batch': 0, 'group_tile_bytes': 0}


class Dev(object):
    """An engine holding a case's matrix with its model set through the C ABI alone (tsem_rowstats -> tsem_set_model)."""

    def __init__(self, gpu_device, c):
        self.c, self.K, self.N = c, c.raw.shape[1], c.raw.shape[0]
        self.eng = eng = _engine(gpu_device)
        raw = c.raw
        eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), self.K, c.M.lut)
        eng.max_score()
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, *c.priors)
        self.col_count = np.asarray(cnt).astype(np.int64)

    def options(self, **kw):
        for key, default in OPTION_DEFAULTS.items():
            self.eng.set_option(key, kw.get(key, default))

    def run(self, method, max_iter, eps=0.0, mult='case', reps=None, seed=0):
        mult = self.c.mult if isinstance(mult, str) else mult
        if reps is not None and mult is not None:
            mult = np.ascontiguousarray(mult[list(reps)])
        n_rep = len(mult) if mult is not None else len(reps)
        return self.eng.bootstrap(n_rep, seed, mult, method, P.CONF, eps, max_iter, self.K)

    def run_groups(self, method, max_iter, eps=0.0):
        return self.eng.bootstrap_groups(len(self.c.mult), 0, self.c.mult, method, P.CONF, eps, max_iter, self.K, keep_values=True)


def _dev(gpu_device, *key):
    if key not in _devs:
        _devs[key] = Dev(gpu_device, P.case(*key))
    d = _devs[key]
    d.options()
    return d


def _fair(ref, label):
    why = ref.fair()
    assert why == [], (label, 'the reference calls this input unfair', why[:5])


def _check(label, got, ref, method, worst=None):
    """checks 1 - 4 for every replicate; returns (and folds into `worst`) the largest error as a fraction of its bound per quantity"""
    worst = {} if worst is None else worst

    def note(name, frac, b, j=0):
        if frac > worst.get(name, (-1.0,))[0]:
            worst[name] = (frac, b, j)
        if not frac <= 1.0:
            _say('%s FAILS: %s of replicate %d at %d: %.4g of its bound', label, name, b, j, frac)
        assert frac <= 1.0, (label, name, 'replicate', b, 'index', j, frac)
    assert len(got['n_frags']) == len(ref.fits), label
    for b, f in enumerate(ref.fits):
        tag = (label, method, 'replicate', b)
        assert int(got['n_frags'][b]) == f.n_frags, tag + ('n_frags', int(got['n_frags'][b]), f.n_frags)
        assert int(got['n_iter'][b]) == f.n_iter and bool(got['converged'][b]) == f.converged, \
            tag + ('n_iter / converged', int(got['n_iter'][b]), f.n_iter, bool(got['converged'][b]), f.converged)
        if f.n_frags == 0:
            assert np.isnan(got['lnl'][b]) and all(np.all(np.isnan(got[k][b])) for k in ('pi', 'theta', 'counts')), tag
            continue
        for name, want, bound in (('pi', f.pi[-1], f.b_pi[-1]), ('theta', f.theta[-1], f.b_theta[-1])):
            v = got[name][b]
            assert not np.any(np.isnan(v)), tag + (name, 'NaN', np.flatnonzero(np.isnan(v))[:5])
            zero = np.flatnonzero((want == 0) != (v == 0))
            assert len(zero) == 0, tag + (name, 'columns that are exactly 0 on one side only', zero[:5])
            frac, j = P.fraction(v, want, bound)
            note(name, frac, b, j)
        frac, _ = P.fraction(got['lnl'][b], f.lnl, f.lnl_limit, absolute=True)
        note('lnl', frac, b)
        cn = got['counts'][b]
        if method in P.INT_METHODS:
            want = f.counts[method].astype(np.float64)
            assert np.array_equal(cn, want), tag + ('counts', np.flatnonzero(cn != want)[:5], cn[cn != want][:5], want[cn != want][:5])
            note('counts_' + method, 0.0, b)
        else:
            frac, j = P.fraction(cn, f.counts[method], f.b_counts[method])
            note('counts_' + method, frac, b, j)
    return worst


def _line(label, worst, **figures):
    _say('%s %s | %s', label, ' '.join('%s=%s' % kv for kv in sorted(figures.items())),
         ' '.join('%s %.3g' % (k, v[0]) for k, v in sorted(worst.items())))


def _ints(got):
    return (got['n_frags'].tolist(), got['n_iter'].tolist(), got['converged'].tolist())


# ---- a. row ranges ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hot', [0, 16, -1])
def test_a_row_ranges(gpu_device, hot):
    """229 rows at 32 / 64 / 96 / 256 / 8192 rows per workgroup: 8, 4, 3, 1 and 1 ranges; the last range holds 5 rows (one trip of 5),
    or ends in a trip of 5; ranges whose first trip is all multiplicity 0 (rows 64 - 95, 192 - 223).  Every hook value against the
    reference; the integer outputs equal across hook values."""
    d = _dev(gpu_device, 'a')
    for t in ITERS:
        ref = d.c.ref(t)
        _fair(ref, ('a', t))
        for method in P.METHODS:
            first, worst = None, {}
            for hook in P.HOOKS:
                d.options(boot_rows_per_block=hook, boot_hot_columns=hot)
                got = d.run(method, t)
                assert got['info'].tolist() == [8, P.K_A if hot < 0 else hot], got['info']
                _check(('a', hot, hook, t), got, ref, method, worst)
                ints = _ints(got) + ((got['counts'].tolist(),) if method in P.INT_METHODS else ())
                first = first or ints
                assert ints == first, ('a', hot, hook, t, method, 'integers differ from those at %d rows per workgroup' % P.HOOKS[0])
            _line('a', worst, hot=hot, iters=t, method=method, hooks=len(P.HOOKS))


@pytest.mark.parametrize('n', [225, 255])
def test_a_last_trip_of_1_and_31_rows(gpu_device, n):
    """the same rows cut to 225 and grown to 255: a last trip of 1 and of 31 rows, at 64 and 256 rows per workgroup"""
    d = _dev(gpu_device, 'a', n)
    for t in ITERS:
        ref = d.c.ref(t)
        _fair(ref, ('a', n, t))
        worst = {}
        for hook in (64, 256):
            for method in P.METHODS:
                d.options(boot_rows_per_block=hook, boot_hot_columns=16)
                _check(('a', n, hook, t), d.run(method, t), ref, method, worst)
        _line('a_last_trip', worst, rows=n, iters=t)


def test_a_hook_refuses_negative_values(gpu_device):
    from telescope_amd._lib import EngineError
    d = _dev(gpu_device, 'a')
    with pytest.raises(EngineError, match='boot_rows_per_block'):
        d.eng.set_option('boot_rows_per_block', -1)
    d.options(boot_rows_per_block=33)                           # rounded up to 64: any value gives the reference's results
    _check(('a', 'hook 33'), d.run('exclude', 2), d.c.ref(2), 'exclude')


# ---- b. the production formula -------------------------------------------------------------------------------------------------------
def test_b_production_formula(gpu_device, cu_count):
    """N = 128 CU + 37 without the hook: rows_per_block = max(32, round_up(ceil(N / (4 CU)), 32)) = 64 on any device — two trips per
    workgroup, the last range short"""
    n = 128 * cu_count + 37
    assert max(32, -(-(-(-n // (4 * cu_count))) // 32) * 32) == 64
    d = _dev(gpu_device, 'b', cu_count)
    ref = d.c.ref(2)
    _fair(ref, 'b')
    worst = {}
    for method in P.METHODS:
        got = d.run(method, 2)
        assert got['info'].tolist() == [8, 300]
        _check('b', got, ref, method, worst)
    _line('b', worst, rows=n, cu=cu_count, iters=2)


# ---- c. row lengths -----------------------------------------------------------------------------------------------------------------
def test_c_row_lengths(gpu_device):
    """rows of 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65 and 255 entries; empty rows first, in the middle and last; rows that store a
    score of 0 (Q = 0 exactly: outside z's pattern)"""
    d = _dev(gpu_device, 'c')
    assert d.c.M.lut[0] == 0.0 and (d.c.raw.data == 0).sum() >= 12
    for t in ITERS:
        ref = d.c.ref(t)
        _fair(ref, ('c', t))
        worst = {}
        for hook, hot in ((0, -1), (64, 0), (96, 16)):
            for method in P.METHODS:
                d.options(boot_rows_per_block=hook, boot_hot_columns=hot)
                _check(('c', hook, hot, t), d.run(method, t), ref, method, worst)
        _line('c', worst, iters=t, zero_scores=int((d.c.raw.data == 0).sum()))


@pytest.mark.parametrize('k', [8, 9])
def test_c_full_rows(gpu_device, k):
    """full rows (b - a == K: no `hole`), one of them a tie of all its entries: at max_iter = 1 the tie is exact on the device —
    exclude gives the row to no column, average an eighth (a ninth) of its multiplicity to each"""
    d = _dev(gpu_device, 'full', k)
    row = d.c.note['tie_row']
    assert d.c.M.lens[row] == k and np.all(d.c.mult[:, row] > 0)
    f = d.c.ref(1).fits[0]
    e = slice(d.c.M.ip[row], d.c.M.ip[row + 1])
    assert np.all(f.assign['exclude'][e] == 0) and np.all(f.assign['average'][e] == LD(1) / k)
    for t in ITERS:
        ref = d.c.ref(t)
        _fair(ref, ('full', k, t))
        worst = {}
        for hot in (0, -1):
            for method in P.METHODS:
                d.options(boot_hot_columns=hot)
                _check(('full', k, hot, t), d.run(method, t), ref, method, worst)
        _line('c_full', worst, K=k, iters=t)


# ---- d. hot columns -----------------------------------------------------------------------------------------------------------------
def _tie_rank(col_count):
    """an H such that the columns of rank H - 1 and H (most popular first, the lower id first among equals) have the same count"""
    order = np.lexsort((np.arange(len(col_count)), -col_count))
    c = col_count[order]
    h = [i for i in range(1, len(c)) if c[i] == c[i - 1] and c[i] > 0]
    assert h, 'no two columns of equal count'
    return h[len(h) // 2], order


def test_d_hot_edges(gpu_device):
    """H = 1, H = K - 1, and an H that falls between two columns of equal col_count (bt_run takes the lower id as the hot one): `info`
    reports H and both columns' sums are right.  Which of the two is hot is not observable from outside: a swapped tie-break would
    pass this leg."""
    d = _dev(gpu_device, 'a')
    h_tie, order = _tie_rank(d.col_count)
    lo, hi = int(order[h_tie - 1]), int(order[h_tie])
    assert lo != hi and d.col_count[lo] == d.col_count[hi]
    for t in ITERS:
        ref = d.c.ref(t)
        worst = {}
        for hot in (1, P.K_A - 1, h_tie):
            for method in P.METHODS:
                d.options(boot_hot_columns=hot, boot_rows_per_block=64)
                got = d.run(method, t)
                assert got['info'].tolist() == [8, hot]
                _check(('d_edges', hot, t), got, ref, method, worst)
        _line('d_edges', worst, iters=t, H_tie=h_tie, cols='%d/%d' % (lo, hi), count=int(d.col_count[lo]))


@pytest.mark.parametrize('n_rep,hot', [(1, 5120), (8, 640)])
def test_d_lds_cap(gpu_device, n_rep, hot):
    """H R = 5120, the most LDS accumulators a workgroup may hold: R = 1 with H = 5120, R = 8 with H = 640, at K = 6000"""
    d = _dev(gpu_device, 'd6000')
    reps = list(range(n_rep))
    for t in ITERS:
        ref = d.c.ref(t, reps=reps)
        _fair(ref, ('d6000', t))
        worst = {}
        for method in P.METHODS:
            d.options(boot_hot_columns=hot, boot_rows_per_block=64)
            got = d.run(method, t, reps=reps)
            assert got['info'].tolist() == [n_rep, hot]
            _check(('d_cap', n_rep, hot, t), got, ref, method, worst)
        _line('d_cap', worst, R=n_rep, H=hot, iters=t)


@pytest.mark.parametrize('hot', [7, 100])
def test_d_small_and_ragged_flush(gpu_device, hot):
    """n_hot = 7 x 3 = 21 (below the 256 threads) and 100 x 3 = 300 (no multiple of 256), 47 row ranges: (blockIdx 67 R) % n_hot wraps
    and the flush index passes n_hot; in replicate 1 every row of one hot column drew 0; replicate 2 has 255 on every row of
    another (both among the `hot` most popular: asserted)"""
    d = _dev(gpu_device, 'd300')
    reps = [0, 1, 2]
    csc = d.c.raw.tocsc()
    zc, hc = d.c.note['zero_col'], d.c.note['heavy_col']
    assert np.all(d.c.mult[1, csc[:, zc].indices] == 0) and np.all(d.c.mult[2, csc[:, hc].indices] == 255)
    top = np.lexsort((np.arange(d.K), -d.col_count))[:hot]             # the hot columns: by (count, id) of the device's own col_count
    assert zc in top and hc in top and csc[:, zc].nnz > 0
    assert (46 * 67 * 3) // (hot * 3) >= 1
    for t in ITERS:
        ref = d.c.ref(t, reps=reps)
        _fair(ref, ('d300', t))
        assert all(ref.fits[1].counts[k][zc] == 0 for k in P.METHODS) and ref.fits[1].pi[-1][zc] == 0
        worst = {}
        for method in P.METHODS:
            d.options(boot_hot_columns=hot, boot_rows_per_block=32)
            got = d.run(method, t, reps=reps)
            assert got['info'].tolist() == [3, hot]
            _check(('d_flush', hot, t), got, ref, method, worst)
        _line('d_flush', worst, H=hot, R=3, iters=t, ranges=47)


# ---- e. batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_rep', [1, 3, 7, 8, 9, 17])
def test_e_batches(gpu_device, n_rep):
    """batches of 1, 3, 7 and 8 replicates; 9 and 17 = full batches and one more, so that rep0 > 0 indexes the explicit
    multiplicities; replicate 4 (and 12) all zeros in the middle of a batch; replicate 6 lives on unique rows only; replicate 2 has
    255 on every row of a hot column"""
    d = _dev(gpu_device, 'd300')
    reps = list(range(n_rep))
    for t in ITERS:
        ref = d.c.ref(t, reps=reps)
        _fair(ref, ('e', n_rep, t))
        if n_rep > 6:
            assert ref.fits[4].n_frags == 0 and ref.fits[6].n_frags > 0 and not np.any(d.c.mult[6][d.c.M.amb])
        worst = {}
        for method in P.METHODS:
            d.options(boot_hot_columns=16)
            got = d.run(method, t, reps=reps)
            assert got['info'].tolist() == [min(8, n_rep), 16]
            _check(('e', n_rep, t), got, ref, method, worst)
        _line('e', worst, n_rep=n_rep, iters=t)


def test_e_staged_stops(gpu_device):
    """one epsilon ends replicate 2 in iteration 1 and replicate 5 in iteration 2 while the others run to 3: the frozen ones keep the
    parameters and the iteration count they stopped with — the reference's of that iteration, and those of the same replicate run
    alone to the same max_iter"""
    d = _dev(gpu_device, 'stop')
    eps = P.stop_eps(d.c)
    ref = d.c.ref(3, eps)
    _fair(ref, 'stop')
    assert [f.n_iter for f in ref.fits] == [3, 3, 1, 3, 3, 2, 3, 3] and ref.fits[2].converged and ref.fits[5].converged
    worst = {}
    for method in P.METHODS:
        got = d.run(method, 3, eps)
        _check('e_stop', got, ref, method, worst)
        for b in (2, 5):
            t = ref.fits[b].n_iter
            alone = d.run(method, t, 0.0, reps=[b])
            _check(('e_stop alone', b), alone, d.c.ref(t, reps=[b]), method, worst)
            assert int(alone['n_iter'][0]) == int(got['n_iter'][b]) == t and int(alone['n_frags'][0]) == int(got['n_frags'][b])
            for name in ('pi', 'theta'):                       # both within the same reference's bounds: at most two bounds apart
                f = ref.fits[b]
                bound = {'pi': f.b_pi[-1], 'theta': f.b_theta[-1]}[name]
                frac, j = P.fraction(got[name][b], alone[name][0].astype(LD), 2 * bound)
                assert frac <= 1.0, ('e_stop', b, name, j, frac)
            if method in P.INT_METHODS:
                assert np.array_equal(alone['counts'][0], got['counts'][b]), ('e_stop', b, method)
    _line('e_stop', worst, eps='%.6g' % eps, n_iter='3,3,1,3,3,2,3,3')


def test_e_default_draws(gpu_device):
    """multiplicities=None: the device draws what synthetic.bootstrap_multiplicities gives (batches of 8 and 1: rep0 > 0 enters the
    hash)"""
    from telescope_amd.synthetic import bootstrap_multiplicities
    d = _dev(gpu_device, 'a')
    seed, n_rep = 11, 9
    mult = np.stack([bootstrap_multiplicities(seed, r, np.arange(d.N)) for r in range(n_rep)])
    for t in ITERS:
        ref = P.BootPass(d.c.raw, mult, d.c.priors, t, M=d.c.M)
        _fair(ref, ('draws', t))
        worst = {}
        for method in P.METHODS:
            d.options(boot_rows_per_block=64)
            got = d.eng.bootstrap(n_rep, seed, None, method, P.CONF, 0.0, t, d.K)
            _check(('e_draws', t), got, ref, method, worst)
        _line('e_draws', worst, iters=t, seed=seed, n_rep=n_rep)


# ---- f. K ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 255, 256, 257])
def test_f_k(gpu_device, k):
    """K = 1, 2, 255, 256, 257: one update block that is not full, exactly full, and a second block of one column; at 257 the
    columns 255 and 256 are twins across the block boundary (twin_rep) and keep identical parameters"""
    d = _dev(gpu_device, 'k', k)
    if k == 257:
        assert d.c.M.twin[256] == 255
    for t in ITERS:
        ref = d.c.ref(t)
        _fair(ref, ('k', k, t))
        worst = {}
        for hot in (0, -1):
            for method in P.METHODS:
                d.options(boot_hot_columns=hot, boot_rows_per_block=64)
                got = d.run(method, t)
                _check(('f', k, hot, t), got, ref, method, worst)
                if k == 257:
                    assert np.array_equal(got['pi'][:, 255], got['pi'][:, 256]) and np.array_equal(got['theta'][:, 255], got['theta'][:, 256])
        _line('f', worst, K=k, iters=t)


def test_f_k_above_65536(gpu_device):
    """K = 65 837: 258 update blocks, so the last block's sum of diff_part takes a second trip.  Most of diff comes from the columns
    from 65 536 on; epsilon lies between iteration 2's diff and its part from the columns below 65 536 — a sum that misses the
    blocks from 256 on stops in iteration 2, the run goes on to 3."""
    d = _dev(gpu_device, 'kbig')
    eps = P.kbig_eps(d.c)
    assert (P.K_BIG + 255) // 256 > 256
    worst = {}
    for t in ITERS:
        ref = d.c.ref(t, eps)
        _fair(ref, ('kbig', t))
        assert all(f.n_iter == t and (t == 3 or not f.converged) for f in ref.fits)
        for method in P.METHODS:
            _check(('f_big', t), d.run(method, t, eps), ref, method, worst)
    _line('f_big', worst, K=P.K_BIG, eps='%.6g' % eps, blocks=(P.K_BIG + 255) // 256)


# ---- g. group sink ------------------------------------------------------------------------------------------------------------------
def _check_groups(label, got, ref, method, worst):
    g = got['groups']
    f0 = ref.fits[0]
    assert np.array_equal(g['group_ptr'], f0.slot_ptr) and np.array_equal(g['cols'], f0.slot_cols), (label, 'the pattern')
    good = np.array([f.n_frags > 0 for f in ref.fits])
    assert g['n_used'] == int(good.sum())
    vals = g['values']
    for b, f in enumerate(ref.fits):
        if not good[b]:
            assert np.all(np.isnan(vals[b])), (label, b)
        elif method in P.INT_METHODS:
            want = f.X[method].astype(np.float64)
            assert np.array_equal(vals[b], want), (label, method, b, np.flatnonzero(vals[b] != want)[:5])
        else:
            frac, j = P.fraction(vals[b], f.X[method], f.b_X[method])
            if frac > worst.get('X_' + method, (-1.0,))[0]:
                worst['X_' + method] = (frac, b, j)
            assert frac <= 1.0, (label, method, b, 'slot', j, frac)
    mean, sd, k = P.welford(vals, good)
    assert np.array_equal(g['mean'].view(np.uint64), mean.view(np.uint64)), (label, method, 'mean is not Welford of the kept values')
    assert np.array_equal(g['sd'].view(np.uint64), sd.view(np.uint64)), (label, method, 'sd is not Welford of the kept values')
    # against the reference's own mean and sd (two passes, long double).  sd is a seminorm: values within e of the reference's move it
    # by sqrt(sum e_b^2 / (B - 1)) at most; Welford's own rounding: B steps on quantities of at most 4 X^2 with a running mean that
    # carries 3 k U X: 16 B^2 U X^2 on M2 — coarse, the bit-for-bit comparison above is the sharp one.
    X = np.array([f.X[method] for f, ok in zip(ref.fits, good) if ok], dtype=LD)
    e = np.array([f.b_X[method] * np.abs(f.X[method]) for f, ok in zip(ref.fits, good) if ok], dtype=LD)
    B = len(X)
    top = np.abs(X).max(0)
    m_ref = X.mean(0)
    m2_ref = ((X - m_ref) ** 2).sum(0)
    frac, j = P.fraction(g['mean'], m_ref, e.max(0) + 4 * B * LD(P.U) * top, absolute=True)
    assert frac <= 1.0, (label, method, 'mean', j, frac)
    m2_dev = (g['sd'].astype(LD) ** 2) * (B - 1)
    lim = 2 * np.sqrt(m2_ref) * np.sqrt((e ** 2).sum(0)) + (e ** 2).sum(0) + (16 * B * B + 4) * LD(P.U) * top ** 2
    frac2, j2 = P.fraction(m2_dev.astype(np.float64), m2_ref, lim, absolute=True)
    assert frac2 <= 1.0, (label, method, 'sd', j2, frac2)
    worst['mean'] = max(worst.get('mean', (0.0,)), (frac, 0, j))
    worst['M2'] = max(worst.get('M2', (0.0,)), (frac2, 0, j2))


@pytest.mark.parametrize('tile', [0, 4096])
def test_g_group_sink(gpu_device, tile):
    """tsem_bootstrap_groups with keep_values on leg a's matrix and hook values: groups of one row (a single-entry row gives a group
    whose column list has one entry), one group of all rows, rows in no group; every slot of every list is compared, the first and
    the last among them; group_tile_bytes 4096 and the default"""
    d = _dev(gpu_device, 'a')
    for name, grp, G in P.group_maps(d.N):
        groups = (grp, G)
        d.eng.set_groups(grp, G)
        for t in ITERS:
            ref = d.c.ref(t, groups=groups)
            f0 = ref.fits[0]
            lens = np.diff(f0.slot_ptr)
            if name == 'one_row':
                assert (lens == 1).any() and f0.slot_ptr[-1] == d.c.M.ip[d.N - 40]
            worst = {}
            for hook in P.HOOKS:
                for method in P.METHODS:
                    d.options(boot_rows_per_block=hook, boot_hot_columns=16, group_tile_bytes=tile)
                    got = d.run_groups(method, t)
                    _check(('g', name, hook, t), got, ref, method, worst)
                    _check_groups(('g', name, hook, t), got, ref, method, worst)
                    if method in P.INT_METHODS:                 # the first and the last slot of every group's list hold what the reference says
                        v = got['groups']['values']
                        full = lens > 0
                        for b in range(len(ref.fits)):
                            for s in (f0.slot_ptr[:-1][full], f0.slot_ptr[1:][full] - 1):
                                assert np.array_equal(v[b][s], ref.fits[b].X[method].astype(np.float64)[s])
            _line('g', worst, map=name, groups=G, slots=int(f0.slot_ptr[-1]), iters=t, tile=tile or 'default')
    d.options()
    d.eng.set_groups(None, 0)
