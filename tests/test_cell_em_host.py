"""`--pooling_mode` on the command line, `CellFits`, and the argument checks of `em_cells` that need no device; plus the closed form
the device unit uses for the columns a cell never touches, checked against the oracle in numpy."""
import os
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import _cell_em_reference as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def test_parser_accepts_pooling_mode_on_both_sc_subcommands():
    from telescope_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf', '--pooling_mode', 'individual'])
    assert a.pooling_mode == 'individual' and cli.pooling_mode(a) == 'individual'
    r = ap.parse_args(['sc', 'resume', 'c.npz', '--pooling_mode', 'pseudobulk'])
    assert r.pooling_mode == 'pseudobulk'
    with pytest.raises(SystemExit):
        ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf', '--pooling_mode', 'celltype'])


def test_default_is_pseudobulk():
    from telescope_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf']).pooling_mode == 'pseudobulk'
    assert ap.parse_args(['sc', 'resume', 'c.npz']).pooling_mode == 'pseudobulk'
    assert cli.pooling_mode(ap.parse_args(['resume', 'c.npz'])) == 'pseudobulk'      # bulk runs have no such option: pooled


@pytest.mark.parametrize('argv', [['assign', 'x.bam', 'y.gtf'], ['resume', 'c.npz']])
def test_parser_rejects_pooling_mode_on_the_bulk_subcommands(argv):
    from telescope_amd import cli
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(argv + ['--pooling_mode', 'individual'])
    assert not hasattr(cli.build_parser().parse_args(argv), 'pooling_mode')


def test_options_list_pooling_mode_only_where_it_exists():
    from telescope_amd import cli
    ap = cli.build_parser()
    sc = str(cli.ResumeOptions(ap.parse_args(['sc', 'resume', 'c.npz', '--pooling_mode', 'individual'])))
    assert 'pooling_mode:' in sc and sc.splitlines()[-1].split() == ['pooling_mode:', 'individual']
    assert 'pooling_mode' not in str(cli.ResumeOptions(ap.parse_args(['resume', 'c.npz'])))


def test_individual_with_updated_sam_is_refused(tmp_path):
    from telescope_amd import cli
    bam, gtf = os.path.join(GOLDEN, 'sc_mixed.bam'), os.path.join(GOLDEN, 'sc_mixed.gtf')
    with pytest.raises(SystemExit) as e:
        cli.main(['sc', 'assign', bam, gtf, '--pooling_mode', 'individual', '--updated_sam', '--skip_em', '--quiet',
                  '--outdir', str(tmp_path)])
    assert 'pooling_mode individual' in str(e.value) and 'updated_sam' in str(e.value)
    assert not os.listdir(str(tmp_path))                     # refused before anything is read or written
    assert cli.main(['sc', 'assign', bam, gtf, '--pooling_mode', 'pseudobulk', '--updated_sam', '--skip_em', '--quiet',
                     '--outdir', str(tmp_path)]) == 0


def _fits():
    from telescope_amd.likelihood import CellFits
    col_ptr = np.array([0, 2, 2, 5])
    cols = np.array([1, 4, 0, 2, 5], np.int32)
    v = np.arange(5, dtype=float)
    rest = np.array([[.1, .2, .3, .4], [.5, .5, np.nan, np.nan], [0., 0., 0., 0.]])
    return CellFits(6, col_ptr, cols, v + 10, v + 20, v + 30, v + 40, rest, [3, 0, 7], [1, 0, 0], [-1., np.nan, -2.])


def test_cell_fits_dense_round_trips():
    f = _fits()
    assert f.n_cells == 3 and f.converged.dtype == bool and list(f.converged) == [True, False, False]
    pi, theta, pi_init, theta_init = f.dense(0)
    assert np.array_equal(pi, [.1, 10, .1, .1, 11, .1]) and np.array_equal(theta, [.2, 20, .2, .2, 21, .2])
    assert np.array_equal(pi_init, [.3, 30, .3, .3, 31, .3]) and np.array_equal(theta_init, [.4, 40, .4, .4, 41, .4])
    pi, theta, pi_init, theta_init = f.dense(1)              # a cell without rows: nothing stored
    assert np.array_equal(pi, np.full(6, .5)) and np.all(np.isnan(pi_init))
    pi, theta, _, _ = f.dense(2)
    assert np.array_equal(pi, [12, 0, 13, 0, 0, 14]) and np.array_equal(theta, [22, 0, 23, 0, 0, 24])
    for c in range(3):                                       # back to the compact form
        a, b = f.col_ptr[c], f.col_ptr[c + 1]
        for dense, compact in zip(f.dense(c), (f.pi, f.theta, f.pi_init, f.theta_init)):
            assert np.array_equal(dense[f.cols[a:b]], compact[a:b])
    with pytest.raises(IndexError):
        f.dense(3)
    with pytest.raises(IndexError):
        f.dense(-1)


def test_cell_fits_rejects_arrays_that_do_not_fit():
    from telescope_amd.likelihood import CellFits
    v = np.zeros(2)
    with pytest.raises(ValueError):
        CellFits(4, [0, 2], np.zeros(2, np.int32), v, v, v, np.zeros(3), np.zeros((1, 4)), [1], [1], [0.])
    with pytest.raises(ValueError):
        CellFits(4, [0, 2], np.zeros(2, np.int32), v, v, v, v, np.zeros((2, 4)), [1], [1], [0.])


class _NoDevice(object):
    """em_cells / select_z up to the point where the device is needed."""

    def __init__(self, n, k, world=1):
        from telescope_amd.likelihood import TelescopeLikelihood, _NullComm
        self.tl = TelescopeLikelihood.__new__(TelescopeLikelihood)
        self.tl.N, self.tl.K = n, k
        self.tl.comm = _NullComm()
        self.tl.comm.world = world
        self.tl._eng = None                                  # any use of the device fails loudly
        self.tl._z, self.tl._z_which, self.tl._report_cache = None, None, {}


def test_em_cells_argument_checks_need_no_device():
    tl = _NoDevice(10, 4).tl
    with pytest.raises(ValueError, match='one entry per row'):
        tl.em_cells(np.zeros(9, np.int32), 2)
    with pytest.raises(ValueError, match='one entry per row'):
        tl.em_cells(np.zeros((10, 1), np.int32), 2)
    with pytest.raises(ValueError, match=r'\[-1, n_cells\)'):
        tl.em_cells(np.full(10, 2, np.int32), 2)
    with pytest.raises(ValueError, match=r'\[-1, n_cells\)'):
        tl.em_cells(np.full(10, -2, np.int32), 2)
    with pytest.raises(NotImplementedError, match='row-sharded'):
        _NoDevice(10, 4, world=2).tl.em_cells(np.zeros(10, np.int32), 1)
    with pytest.raises(ValueError, match='no per-cell posteriors'):
        tl.select_z('cells')
    with pytest.raises(ValueError, match='no pooled posteriors'):
        tl.select_z('pooled')
    with pytest.raises(ValueError):
        tl.select_z('both')


def test_header_declares_and_library_lists_the_unit():
    from telescope_amd import _lib
    assert 'tsem_cellem' in _lib.LIB_UNITS
    for name in ('tsem_cell_em', 'tsem_cell_em_shape', 'tsem_cell_em_copy'):
        assert name in _lib.exported_symbols()


def test_boundary_matrix_gives_every_cell_its_columns_and_entries():
    cells = [(5, 5), (1, 9), (7, 40), (64, 64)]
    raw, cor, cols = R.boundary_matrix(11, 64, cells)
    assert raw.has_canonical_format and raw.shape[1] == 64 and raw.nnz == sum(ne for _, ne in cells)
    lens = np.diff(raw.indptr)
    assert lens.min() >= 1 and lens.max() <= 8 and raw.data.min() >= 100 and raw.data.max() <= 399
    for c, (kc, ne) in enumerate(cells):
        sub = raw[cor == c]
        assert sub.nnz == ne and len(cols[c]) == kc and np.array_equal(np.unique(sub.indices), cols[c]), c
        assert np.diff(sub.indptr).max() <= kc
    assert np.any(np.diff(cor) < 0)                          # (the cells' rows are shuffled together)
    again = R.boundary_matrix(11, 64, cells)
    assert np.array_equal(again[0].data, raw.data) and np.array_equal(again[1], cor)


def test_boundary_case_is_decided_by_no_rounding():
    """What tests/test_gpu_cell_em_edges.py relies on in case B, from the oracle alone: every cell has the column and entry counts
    that put it where the case says; every cell is fitted without a NaN, in 2 to 100 iterations; the rows the oracle cannot decide
    stay under the 0.5 % cap of the count comparison; and no iteration's stop test — diff, or the step of lnl — lies within 1e-6
    relative of epsilon, so that iteration counts can be compared for equality."""
    raw, cor, cols = R.boundary_case()
    assert raw.shape[1] == R.B_K
    want = [0, 0, 0, 0]
    for c, (kc, ne) in enumerate(R.B_CELLS):
        sub = raw[cor == c]
        assert sub.nnz == ne and np.array_equal(np.unique(sub.indices), cols[c]) and len(cols[c]) == kc, c
        want[0 if (kc <= 256 and ne <= 4096) else 1 if kc <= 1024 else 2 if kc <= 3840 else 3] += 1
    assert tuple(want) == R.B_CLASSES
    for params in R.B_PARAMS:
        ref = R.cell_ref('B', *params)
        for c, om in enumerate(ref.fits):
            assert om is not None and 2 <= om.n_iter <= R.MAX_ITER, (params, c)
            assert not np.any(np.isnan(om.pi)) and not np.any(np.isnan(om.theta)) and not np.isnan(om.lnl), (params, c)
        assert len(ref.undecided_rows()) <= 0.005 * ref.fitted_rows(), params
        assert R.stop_margin(ref) > 1e-6, (params, R.stop_margin(ref))
    assert R.stop_margin(R.cell_ref('large', 0, 200000)) > 1e-6


@pytest.mark.parametrize('pi_prior,theta_prior,use_likelihood', [(0, 200000, False), (0, 0, False), (1, 5, True)])
def test_closed_form_of_untouched_columns_equals_the_oracle(pi_prior, theta_prior, use_likelihood):
    """The fit on a cell's compacted columns — one closed-form value for the K - Kc columns the cell never touches, which count in
    diff — is the oracle's fit of the cell on all K columns: same iteration count, parameters and lnl at 1e-9."""
    from oracle.telescope_oracle import OracleModel
    from telescope_amd.likelihood import score_lut
    raw, cor = R.random_matrix(3, 900, 400, 6)
    lut = score_lut(raw.max())
    for c in range(6):
        rows = np.flatnonzero(cor == c)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            om = OracleModel(raw[rows], pi_prior, theta_prior, max_score=raw.max())
            om.em(R.EPSILON, R.MAX_ITER, use_likelihood)
            cols, pi, th, rp, rt, it, conv, lnl = R.emulate_cell(raw[rows], lut, raw.shape[1], pi_prior, theta_prior, R.EPSILON,
                                                                 R.MAX_ITER, use_likelihood)
        assert len(cols) < raw.shape[1]
        assert it == om.n_iter and bool(conv) == bool(om.converged)
        dpi, dth = np.full(raw.shape[1], rp), np.full(raw.shape[1], rt)
        dpi[cols], dth[cols] = pi, th
        assert np.allclose(dpi, om.pi, rtol=R.RTOL, atol=0) and np.allclose(dth, om.theta, rtol=R.RTOL, atol=0)
        assert np.isclose(lnl, om.lnl, rtol=R.RTOL, atol=0)
