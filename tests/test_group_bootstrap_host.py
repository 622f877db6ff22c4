"""The per-group bootstrap without a device: its reference (tests/_group_bootstrap_reference.py) against the bulk reference it builds
on, the Welford update against numpy's moments, `--bootstrap_ci` on the bulk commands and the writers of the mean / sd tables."""
import os
import types

import numpy as np
import pytest
import scipy.sparse as sp

import _bootstrap_reference as B
import _group_bootstrap_reference as GB
from _bootstrap_reference import RTOL


def _fair(ref):
    assert ref.undecided() == 0
    assert ref.stop_margin() > 1e-6, ref.stop_margin()


def test_group_values_add_up_to_the_replicate_counts():
    """On C2: the groups' values plus the part of the rows in no group are the replicate's counts — exactly for the integer methods."""
    ref = B.case_ref('C2')
    _fair(ref)
    n, g = ref.N, 12
    cor = GB.random_map(11, n, g, empty=(0, 5, 11))
    assert (cor < 0).any() and set(np.unique(cor[cor >= 0])) == set(range(g)) - {0, 5, 11}
    gptr, cols = GB.structural_pattern(ref.raw, cor, g)
    assert gptr[1] == 0 and gptr[6] == gptr[5] and gptr[12] == gptr[11] == len(cols)
    for method in B.METHODS:
        for b in range(len(B.REPS)):
            x = GB.group_values(ref, b, method, cor, g)
            assert x.shape == (g, ref.K)
            total = x.sum(0) + GB.ungrouped_counts(ref, b, method, cor)
            want = ref.counts(b, method)
            if method in B.INT_METHODS:
                assert np.array_equal(total, want), (method, b)
                assert np.array_equal(x, np.rint(x))
            else:
                assert np.allclose(total, want, rtol=RTOL, atol=RTOL * want.max()), (method, b)
            dense = np.zeros_like(x)                           # nothing lies outside the structural pattern
            grp = np.repeat(np.arange(g), np.diff(gptr))
            dense[grp, cols] = GB.on_pattern(x, gptr, cols)
            assert np.array_equal(dense, x), (method, b)


def test_welford_equals_numpy_moments():
    rng = np.random.RandomState(2)
    vals = np.concatenate([rng.poisson(3., (9, 40)).astype(float), rng.rand(9, 40) * 1e3, 1e6 + rng.rand(9, 40)], axis=1)
    for good in (np.ones(9, bool), np.array([1, 0, 1, 1, 0, 1, 1, 1, 0], bool)):
        mean, sd = GB.welford(vals, good)
        wm, ws = GB.moments(vals, good)
        atol = RTOL * np.abs(wm).max()
        assert np.allclose(mean, wm, rtol=RTOL, atol=atol) and np.allclose(sd, ws, rtol=RTOL, atol=atol)
        GB.assert_moments(mean, sd, wm, ws)
    const = np.tile(rng.rand(1, 7) * 100, (6, 1))
    mean, sd = GB.welford(const, np.ones(6, bool))
    assert np.array_equal(mean, const[0]) and np.all(sd == 0.)
    mean, sd = GB.welford(vals, np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], bool))
    assert np.array_equal(mean, vals[2]) and np.all(np.isnan(sd))
    wm, ws = GB.moments(vals, np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], bool))
    assert np.array_equal(wm, vals[2]) and np.all(np.isnan(ws))
    mean, sd = GB.welford(vals, np.zeros(9, bool))
    assert np.all(np.isnan(mean)) and np.all(np.isnan(sd))
    wm, ws = GB.moments(vals, np.zeros(9, bool))
    assert np.all(np.isnan(wm)) and np.all(np.isnan(ws))


# ---- the command line: the level of the bounds (the `sc` sub-commands keep refusing the bootstrap options, tests/test_bootstrap_host.py) ----
MISSING = os.path.join(os.sep, 'nonexistent', 'dir')
BULK = {'resume': ['resume', os.path.join(MISSING, 'x.npz')],
        'assign': ['assign', os.path.join(MISSING, 'x.bam'), os.path.join(MISSING, 'y.gtf')]}


@pytest.mark.parametrize('form', sorted(BULK))
def test_bulk_parsers_take_the_level(form):
    from telescope_amd import cli
    ap = cli.build_parser()
    assert ap.parse_args(BULK[form]).bootstrap_ci == 0.95
    a = ap.parse_args(BULK[form] + ['--bootstrap', '5', '--bootstrap_seed', '2', '--bootstrap_ci', '0.9'])
    assert (a.bootstrap, a.bootstrap_seed, a.bootstrap_ci) == (5, 2, 0.9)
    cli._refuse_bootstrap(a)


@pytest.mark.parametrize('form', sorted(BULK))
@pytest.mark.parametrize('level', ['1.5', '0', '1', '-0.1', 'nan'])
def test_a_level_outside_the_unit_interval_is_refused(form, level, tmp_path):
    from telescope_amd import cli
    with pytest.raises(SystemExit) as e:
        cli.main(BULK[form] + ['--bootstrap', '4', '--bootstrap_ci', level, '--outdir', str(tmp_path / 'out')])
    assert isinstance(e.value.code, str) and '--bootstrap_ci' in e.value.code
    assert not (tmp_path / 'out').exists()


def test_the_level_reaches_the_bootstrap_table():
    import io
    from telescope_amd.likelihood import BootstrapFits
    from telescope_amd.run_container import write_bootstrap_tsv
    rng = np.random.RandomState(4)
    b, k = 20, 3
    fits = BootstrapFits(rng.rand(b, k), rng.rand(b, k), rng.poisson(30., (b, k)).astype(float), np.full(b, 100), np.full(b, 7), np.ones(b),
                         rng.rand(b), seed=1)
    out = {}
    for level in (0.95, 0.8):
        fh = io.StringIO()
        write_bootstrap_tsv(fh, ['a', 'b', 'c'], np.arange(3), fits, level)
        out[level] = fh.getvalue().splitlines()
        assert 'level:%g' % level in out[level][0].split('\t')
    lo95, hi95 = (np.array([float(l.split('\t')[i]) for l in out[0.95][2:]]) for i in (4, 5))
    lo80, hi80 = (np.array([float(l.split('\t')[i]) for l in out[0.8][2:]]) for i in (4, 5))
    assert np.all(lo95 <= lo80) and np.all(hi80 <= hi95) and (np.any(lo95 < lo80) or np.any(hi80 < hi95))
    want = np.quantile(fits.counts, [0.1, 0.9], axis=0)
    assert np.allclose(lo80, want[0], atol=0.005) and np.allclose(hi80, want[1], atol=0.005)    # (printed with two decimals)


# ---- the writers ----
def _hand_made():
    """3 cells x 5 loci: cell 1 is empty, one slot has sd 0 (and one mean 0: a slot no replicate ever counted)"""
    from telescope_amd.likelihood import BootstrapCells
    gptr = np.array([0, 3, 3, 5])
    cols = np.array([0, 2, 4, 1, 2], np.int32)
    mean = np.array([1.5, 2.0, 0.0, 0.25, 7.0])
    sd = np.array([0.5, 0.0, 0.0, 0.125, 1.0 / 3.0])
    return BootstrapCells(3, 5, gptr, cols, mean, sd, 4)


def _container(fmt):
    from telescope_amd.run_container import scTelescope
    ts = scTelescope(types.SimpleNamespace(count_format=fmt))
    ts.barcodes = ['AAAC', 'CCCG', 'GGGT']
    ts.feat_index = {'__no_feature': 0, 'L1': 1, 'L2': 2, 'L3': 3, 'L4': 4}
    return ts


def test_cells_class_gives_sparse_matrices():
    c = _hand_made()
    m, s = c.mean_matrix(), c.sd_matrix()
    assert m.shape == s.shape == (3, 5) and m.nnz == 4 and s.nnz == 3                    # zeros are dropped
    assert np.array_equal(m.toarray(), [[1.5, 0, 2.0, 0, 0], [0] * 5, [0, 0.25, 7.0, 0, 0]])
    assert np.array_equal(s.toarray(), [[0.5, 0, 0, 0, 0], [0] * 5, [0, 0.125, 1.0 / 3.0, 0, 0]])
    assert c.values is None and c.n_used == 4 and c.nnz == 5
    with pytest.raises(ValueError, match='keep_replicates'):
        c.values_matrix(0)
    from telescope_amd.likelihood import BootstrapCells
    k = BootstrapCells(3, 5, c.group_ptr, c.cols, c.mean, c.sd, 2, np.arange(10.).reshape(2, 5))
    assert np.array_equal(k.values_matrix(1).toarray(), [[5, 0, 6, 0, 7], [0] * 5, [0, 8, 9, 0, 0]])
    assert k.values_matrix(0).nnz == 4
    with pytest.raises(ValueError):
        BootstrapCells(3, 5, c.group_ptr, c.cols[:-1], c.mean, c.sd, 2)


def test_writers_tsv(tmp_path):
    ts = _container('tsv')
    fits = types.SimpleNamespace(cells=_hand_made())
    mean, sd = tmp_path / 't-TE_counts_boot_mean.tsv', tmp_path / 't-TE_counts_boot_sd.tsv'
    ts.output_cell_bootstrap(fits, str(mean), str(sd))
    assert sorted(os.listdir(str(tmp_path))) == ['t-TE_counts_boot_mean.tsv', 't-TE_counts_boot_sd.tsv']
    assert mean.read_text() == ('\t__no_feature\tL1\tL2\tL3\tL4\n' 'AAAC\t1.5\t0.0\t2.0\t0.0\t0.0\n' 'CCCG\t0.0\t0.0\t0.0\t0.0\t0.0\n'
                                'GGGT\t0.0\t0.25\t7.0\t0.0\t0.0\n')
    assert sd.read_text() == ('\t__no_feature\tL1\tL2\tL3\tL4\n' 'AAAC\t0.5\t0.0\t0.0\t0.0\t0.0\n' 'CCCG\t0.0\t0.0\t0.0\t0.0\t0.0\n'
                              'GGGT\t0.0\t0.125\t0.3333333333333333\t0.0\t0.0\n')


def test_writers_mtx(tmp_path):
    import scipy.io
    ts = _container('mtx')
    fits = types.SimpleNamespace(cells=_hand_made())
    ts.output_cell_bootstrap(fits, str(tmp_path / 't-TE_counts_boot_mean.tsv'), str(tmp_path / 't-TE_counts_boot_sd.tsv'))
    assert sorted(os.listdir(str(tmp_path))) == ['t-TE_counts_boot_mean.mtx', 't-TE_counts_boot_sd.mtx', 't-barcodes.tsv', 't-features.tsv']
    m = scipy.io.mmread(str(tmp_path / 't-TE_counts_boot_mean.mtx'))
    s = scipy.io.mmread(str(tmp_path / 't-TE_counts_boot_sd.mtx'))
    assert np.array_equal(m.toarray(), fits.cells.mean_matrix().toarray()) and np.array_equal(s.toarray(), fits.cells.sd_matrix().toarray())
    assert sp.coo_matrix(s).nnz == 3
    assert (tmp_path / 't-barcodes.tsv').read_text().split() == ts.barcodes
    assert (tmp_path / 't-features.tsv').read_text().split() == ['__no_feature', 'L1', 'L2', 'L3', 'L4']
