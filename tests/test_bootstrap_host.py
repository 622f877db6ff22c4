"""`--bootstrap` on the command line, `BootstrapFits`, the bootstrap TSV, the default multiplicities and the argument checks of
`TelescopeLikelihood.bootstrap` that need no device; plus the weighted closed form the device unit evaluates, held in numpy against
the definition of a replicate: the oracle's fit of the matrix with every row repeated by its multiplicity."""
import io
import math
import os

import numpy as np
import pytest

import _bootstrap_reference as B
from _bootstrap_reference import RTOL

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CHECKPOINT = os.path.join(GOLDEN, 'resume_checkpoint.npz')


# ---- default multiplicities ----------------------------------------------------------------------------------------------------
def test_multiplicities_are_deterministic_and_differ_by_replicate_and_seed():
    from telescope_amd.synthetic import bootstrap_multiplicities
    rows = np.arange(5000)
    a = bootstrap_multiplicities(7, 0, rows)
    assert np.array_equal(a, bootstrap_multiplicities(7, 0, rows))
    assert np.array_equal(a[100:200], bootstrap_multiplicities(7, 0, rows[100:200]))      # a function of the row alone
    assert not np.array_equal(a, bootstrap_multiplicities(7, 1, rows))
    assert not np.array_equal(a, bootstrap_multiplicities(8, 0, rows))


def test_multiplicities_are_poisson_one_draws():
    from telescope_amd.synthetic import bootstrap_multiplicities, poisson_cdf_u32
    m = bootstrap_multiplicities(3, 2, np.arange(100000))
    assert m.dtype == np.uint8 and m.max() <= 14 and len(poisson_cdf_u32(1.0)) == 14
    assert abs((m == 0).mean() - math.exp(-1)) < 0.01
    assert abs(m.mean() - 1.0) < 0.01


def test_multiplicities_follow_the_documented_expression():
    from telescope_amd import synthetic as S
    rows = np.arange(1000, 1300)
    h = (S.hash3(np.uint64(11) ^ S.SALT_BOOT, rows, 4) >> np.uint64(32)).astype(np.uint32)
    t = S.poisson_cdf_u32(1.0)
    want = np.array([(t <= x).sum() for x in h], dtype=np.uint8)
    assert np.array_equal(S.bootstrap_multiplicities(11, 4, rows), want)


# ---- the definition --------------------------------------------------------------------------------------------------------------
def test_weighted_closed_form_equals_the_oracle_on_repeated_rows():
    """Case C2: the weighted EM over the whole matrix is the oracle's fit of the resampled matrix — iteration counts equal, pi,
    theta and lnl at RTOL, integer counts equal, float counts at RTOL."""
    ref = B.case_ref('C2')
    raw = B.case_matrix('C2')
    _, _, _, pp, tp = B.CASES['C2']
    assert ref.undecided() == 0 and ref.stop_margin() > 1e-6
    for b, om in enumerate(ref.fits):
        for method in B.METHODS:
            got = B.weighted_fit(raw, ref.mult[b], pp, tp, method=method)
            assert got['n_iter'] == om.n_iter and got['converged'] == bool(om.converged), (b, got['n_iter'], om.n_iter)
            assert got['n_frags'] == om.N
            assert np.allclose(got['pi'], om.pi, rtol=RTOL, atol=0) and np.allclose(got['theta'], om.theta, rtol=RTOL, atol=0), b
            assert np.isclose(got['lnl'], om.lnl, rtol=RTOL, atol=0), (b, got['lnl'], om.lnl)
            want = ref.counts(b, method)
            if method in B.INT_METHODS:
                assert np.array_equal(got['counts'], want), (b, method)
            else:
                assert np.allclose(got['counts'], want, rtol=RTOL, atol=0), (b, method)


def test_weighted_closed_form_without_fragments_is_not_fitted():
    raw = B.case_matrix('C2')
    got = B.weighted_fit(raw, np.zeros(raw.shape[0], np.uint8), 1, 5)
    assert got['n_iter'] == 0 and not got['converged'] and np.isnan(got['lnl']) and np.all(np.isnan(got['pi']))


# ---- the parser --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('argv', [['assign', 'x.bam', 'y.gtf'], ['resume', 'c.npz']])
def test_parser_has_the_options_on_the_bulk_subcommands(argv):
    from telescope_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(argv)
    assert a.bootstrap == 0 and a.bootstrap_seed == 0
    a = ap.parse_args(argv + ['--bootstrap', '32', '--bootstrap_seed', '5'])
    assert a.bootstrap == 32 and a.bootstrap_seed == 5


@pytest.mark.parametrize('argv', [['sc', 'assign', 'x.bam', 'y.gtf'], ['sc', 'resume', 'c.npz']])
def test_parser_has_no_bootstrap_on_the_sc_subcommands(argv):
    from telescope_amd import cli
    ap = cli.build_parser()
    assert not hasattr(ap.parse_args(argv), 'bootstrap') and not hasattr(ap.parse_args(argv), 'bootstrap_seed')
    with pytest.raises(SystemExit):
        ap.parse_args(argv + ['--bootstrap', '4'])
    with pytest.raises(SystemExit):
        ap.parse_args(argv + ['--bootstrap_seed', '4'])


def test_options_block_does_not_list_the_new_keys():
    from telescope_amd import cli
    text = str(cli.ResumeOptions(cli.build_parser().parse_args(['resume', 'c.npz', '--bootstrap', '4'])))
    assert 'bootstrap' not in text


@pytest.mark.parametrize('extra,env,words', [
    (['--reassign_mode', 'choose'], {}, ('--bootstrap', 'choose')),
    (['--use_likelihood'], {}, ('--bootstrap', '--use_likelihood')),
    (['--reproducible'], {}, ('--bootstrap', '--reproducible')),
    ([], {'WORLD_SIZE': '2'}, ('--bootstrap', 'WORLD_SIZE')),
])
def test_refusals_come_before_anything_is_read_or_written(tmp_path, monkeypatch, extra, env, words):
    from telescope_amd import cli
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    out = tmp_path / 'out'
    out.mkdir()
    with pytest.raises(SystemExit) as e:
        cli.main(['resume', CHECKPOINT, '--bootstrap', '4', '--skip_em', '--quiet', '--outdir', str(out)] + extra)
    assert all(w in str(e.value) for w in words), str(e.value)
    assert not os.listdir(str(out))
    with pytest.raises(SystemExit):                           # ... whatever the checkpoint: it is never opened
        cli.main(['resume', str(tmp_path / 'missing.npz'), '--bootstrap', '4', '--quiet', '--outdir', str(out)] + extra)
    assert not os.listdir(str(out))
    with pytest.raises(SystemExit):
        cli.main(['assign', str(tmp_path / 'missing.bam'), str(tmp_path / 'missing.gtf'), '--bootstrap', '4', '--quiet', '--outdir', str(out)] + extra)
    assert not os.listdir(str(out))


def test_without_bootstrap_the_same_options_are_not_refused(tmp_path):
    from telescope_amd import cli
    assert cli.main(['resume', CHECKPOINT, '--skip_em', '--quiet', '--reassign_mode', 'choose', '--use_likelihood', '--reproducible',
                     '--outdir', str(tmp_path)]) == 0


# ---- BootstrapFits and the TSV ---------------------------------------------------------------------------------------------------
def _fits():
    """Four replicates over three loci; replicate 2 has no fragments (not fitted), replicate 3 has NaN parameters."""
    from telescope_amd.likelihood import BootstrapFits
    nan = np.nan
    pi = np.array([[.5, .3, .2], [.6, .3, .1], [nan, nan, nan], [nan, nan, nan], [.4, .3, .3]])
    theta = np.where(np.isnan(pi), nan, .25)
    counts = np.array([[10., 4., 0.], [12., 4., 1.], [nan, nan, nan], [nan, nan, nan], [8., 4., 2.]])
    return BootstrapFits(pi, theta, counts, [20, 22, 0, 5, 18], [7, 9, 0, 100, 100], [1, 1, 0, 0, 0], [-1., -2., nan, nan, -3.],
                         info={'batch': 5, 'hot_columns': 3}, seed=3, method='average')


def test_fitted_skips_replicates_without_fragments_or_with_nan_parameters():
    f = _fits()
    assert f.n_rep == 5 and f.K == 3 and f.converged.dtype == bool
    assert list(f.fitted) == [True, True, False, False, True]
    assert f.info == {'batch': 5, 'hot_columns': 3}


def test_summary_takes_mean_sd_and_quantiles_over_the_fitted_replicates():
    f = _fits()
    s = f.summary(0.95)
    keep = [0, 1, 4]
    for key, a in (('counts', f.counts), ('pi', f.pi)):
        assert np.array_equal(s[key]['mean'], a[keep].mean(0))
        assert np.array_equal(s[key]['sd'], a[keep].std(0, ddof=1))
        assert np.allclose(s[key]['lo'], np.quantile(a[keep], 0.025, axis=0), rtol=1e-12, atol=0)    # ((1 - 0.95) / 2 is not 0.025 to the bit)
        assert np.allclose(s[key]['hi'], np.quantile(a[keep], 0.975, axis=0), rtol=1e-12, atol=0)
    assert np.allclose(s['counts']['mean'], [10., 4., 1.]) and np.allclose(s['counts']['sd'], [2., 0., 1.])
    s50 = f.summary(0.5)
    assert np.array_equal(s50['counts']['lo'], np.quantile(f.counts[keep], 0.25, axis=0))
    with pytest.raises(ValueError):
        f.summary(1.0)


def test_summary_with_one_or_no_fitted_replicate():
    from telescope_amd.likelihood import BootstrapFits
    one = BootstrapFits([[.5, .5]], [[.5, .5]], [[3., 1.]], [4], [5], [1], [-1.])
    s = one.summary()
    assert np.array_equal(s['counts']['mean'], [3., 1.]) and np.all(np.isnan(s['counts']['sd'])) and np.array_equal(s['pi']['lo'], [.5, .5])
    none = BootstrapFits([[np.nan, np.nan]], [[np.nan, np.nan]], [[np.nan, np.nan]], [0], [0], [0], [np.nan])
    assert not none.fitted.any() and all(np.all(np.isnan(v)) for v in none.summary()['pi'].values())
    with pytest.raises(ValueError):
        BootstrapFits([[.5, .5]], [[.5, .5]], [[3., 1.]], [4, 4], [5], [1], [-1.])


def test_tsv_writer():
    from telescope_amd.run_container import write_bootstrap_tsv
    f = _fits()
    fh = io.StringIO()
    write_bootstrap_tsv(fh, ['locB', 'locA', 'locC'], np.array([9.5, 4., 1.]), f)
    lines = fh.getvalue().splitlines()
    assert lines[0] == '## Bootstrap\treplicates:5\tseed:3\tfitted:3\tconverged:2\tmethod:average\tlevel:0.95'
    assert lines[1].split('\t') == ['transcript', 'count', 'count_mean', 'count_sd', 'count_lo', 'count_hi', 'prop_mean', 'prop_sd',
                                    'prop_lo', 'prop_hi']
    assert [l.split('\t')[0] for l in lines[2:]] == ['locA', 'locB', 'locC']           # sorted like TE_counts.tsv
    s = f.summary()
    row = lines[3].split('\t')                                                        # locB = column 0
    assert row[1] == '9.5'
    assert row[2:6] == ['%.2f' % s['counts'][k][0] for k in ('mean', 'sd', 'lo', 'hi')] and row[2] == '10.00' and row[3] == '2.00'
    assert row[6:10] == ['%.6g' % s['pi'][k][0] for k in ('mean', 'sd', 'lo', 'hi')] and row[6] == '0.5'
    assert len(lines) == 5
    fh = io.StringIO()                                                                # integer counts print as TE_counts.tsv prints them
    write_bootstrap_tsv(fh, ['a', 'b', 'c'], np.array([9, 4, 1], dtype=np.int64), f)
    assert [l.split('\t')[1] for l in fh.getvalue().splitlines()[2:]] == ['9', '4', '1']


# ---- argument checks that need no device -------------------------------------------------------------------------------------------
class _NoDevice(object):
    def __init__(self, n, k, world=1):
        from telescope_amd.likelihood import TelescopeLikelihood, _NullComm
        self.tl = TelescopeLikelihood.__new__(TelescopeLikelihood)
        self.tl.N, self.tl.K = n, k
        self.tl.comm = _NullComm()
        self.tl.comm.world = world
        self.tl._eng = None                                  # any use of the device fails loudly
        self.tl.epsilon, self.tl.max_iter = 1e-7, 100


def test_bootstrap_argument_checks_need_no_device():
    tl = _NoDevice(10, 4).tl
    with pytest.raises(ValueError, match='choose'):
        tl.bootstrap(4, method='choose')
    with pytest.raises(ValueError) as e:
        tl.bootstrap(4, method='best')
    assert str(e.value) == 'Argument "method" should be one of (exclude, choose, average, conf, unique, all)'
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match='n_rep'):
            tl.bootstrap(bad)
    with pytest.raises(ValueError, match='shape'):
        tl.bootstrap(2, multiplicities=np.ones((2, 9), np.uint8))
    with pytest.raises(ValueError, match='shape'):
        tl.bootstrap(2, multiplicities=np.ones((3, 10), np.uint8))
    with pytest.raises(ValueError, match='shape'):
        tl.bootstrap(2, multiplicities=np.ones(20, np.uint8))
    with pytest.raises(ValueError, match='uint8'):
        tl.bootstrap(2, multiplicities=np.ones((2, 10), np.int64))
    with pytest.raises(NotImplementedError, match='row-sharded'):
        _NoDevice(10, 4, world=2).tl.bootstrap(2)
    with pytest.raises(AttributeError):                      # valid arguments reach the device (there is none here)
        tl.bootstrap(2, multiplicities=np.ones((2, 10), np.uint8))


def test_header_declares_and_library_lists_the_unit():
    from telescope_amd import _lib
    assert 'tsem_boot' in _lib.LIB_UNITS
    for name in ('tsem_bootstrap', 'tsem_bootstrap_copy', 'tsem_bootstrap_mult'):
        assert name in _lib.exported_symbols()
