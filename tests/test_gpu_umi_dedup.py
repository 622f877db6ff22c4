"""tsem_umi_dedup on the device against the plain host definition (tests/_umi_reference.py): `rep` and `stats` are compared for
equality.  Random cases, edge cases, the same result whatever else the handle holds, the handle's state untouched, the refusals, and
`sc assign --umi_tag` / `sc resume` end to end against plain runs of the collapsed matrix.

The engine takes canonical CSR only (tsem_load_scores refuses column ids that do not ascend inside a row), so a case whose column
ids are in no order is given to the REFERENCE as it is and to the device with every row's ids sorted: the definition does not depend
on their order, which tests/test_umi_reference.py holds on the host."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from _umi_reference import dedup_plain, ground, random_case
from conftest import GOLD, Opts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _canonical(indptr, indices, data, k):
    m = sp.csr_matrix((np.asarray(data, np.uint16), np.asarray(indices, np.int32), np.asarray(indptr, np.int64)), shape=(len(indptr) - 1, k))
    m.sort_indices()
    return m


def _engine(indptr, indices, data, k, options=None):
    from telescope_amd import _lib
    m = _canonical(indptr, indices, data, k)
    eng = _lib.Engine(0)
    for key, v in (options or {}).items():
        eng.set_option(key, v)
    eng.load_scores(m.indptr, m.indices, m.data, k, None)
    return eng


def _device(indptr, indices, data, k, cell, umi, n_cells=None, n_umis=None):
    eng = _engine(indptr, indices, data, k)
    try:
        return eng.umi_dedup(cell, umi, int(np.max(cell, initial=-1)) + 1 if n_cells is None else n_cells,
                             int(np.max(umi, initial=-1)) + 1 if n_umis is None else n_umis)
    finally:
        eng.close()


def _check(indptr, indices, data, k, cell, umi, n_cells=None, n_umis=None):
    want_rep, want_stats = dedup_plain(indptr, indices, data, cell, umi)
    rep, stats = _device(indptr, indices, data, k, cell, umi, n_cells, n_umis)
    assert rep.dtype == np.int32 and stats.dtype == np.int64
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    assert np.array_equal(rep, want_rep), np.flatnonzero(rep != want_rep)[:10]
    return rep, stats


_RANDOM = {}


def _random(seed):
    """one random case and its reference, computed once"""
    if seed not in _RANDOM:
        c = random_case(seed)
        _RANDOM[seed] = (c, dedup_plain(*c[:5]))
    return _RANDOM[seed]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_cases(gpu_device, seed):
    (indptr, indices, data, cell, umi, k), (want_rep, want_stats) = _random(seed)
    assert len(indptr) - 1 == 3000 and k == 60 and cell.min() == -1 and cell.max() == 11 and umi.min() == -1 and umi.max() == 39
    assert any(np.any(np.diff(indices[indptr[i]:indptr[i + 1]]) < 0) for i in range(100))      # column ids in no order
    dropped, big, split = ground(indptr, indices, data, cell, umi)
    assert dropped >= 500 and big >= 100 and split >= 200, (dropped, big, split)
    rep, stats = _device(indptr, indices, data, k, cell, umi, 12, 40)
    assert np.array_equal(stats, want_stats), (stats, want_stats)
    assert np.array_equal(rep, want_rep), np.flatnonzero(rep != want_rep)[:10]


def _one_class(n):
    return np.zeros(n, np.int32), np.zeros(n, np.int32)


def test_chain_of_300_rows_is_one_component(gpu_device):
    n = 300
    indptr = 2 * np.arange(n + 1, dtype=np.int64)
    indices = np.stack([np.arange(n), np.arange(n) + 1], 1).ravel().astype(np.int32)
    data = (1 + (np.arange(2 * n) * 7) % 50).astype(np.uint16)       # the largest code, 50, is met several times: the smallest row wins
    cell, umi = _one_class(n)
    rep, stats = _check(indptr, indices, data, n + 1, cell, umi)
    first = int(np.flatnonzero(data.reshape(n, 2).max(1) == 50)[0])
    assert np.all(rep == first) and stats.tolist() == [n, 1, 1, n - 1]


def test_5000_rows_on_one_column(gpu_device):
    n = 5000
    rng = np.random.default_rng(5)
    indptr = np.arange(n + 1, dtype=np.int64)
    indices = np.zeros(n, np.int32)
    data = rng.integers(1, 400, n).astype(np.uint16)
    rep, stats = _check(indptr, indices, data, 3, *_one_class(n))
    assert np.all(rep == int(np.argmax(data))) and stats.tolist() == [n, 1, 1, n - 1]


def test_rows_of_1500_entries(gpu_device):
    rng = np.random.default_rng(6)
    k, ln = 3200, 1500
    cols = [rng.permutation(1600)[:ln], rng.permutation(1600)[:ln], 1600 + rng.permutation(1600)[:ln], 1600 + rng.permutation(1600)[:ln],
            rng.permutation(k)[:3]]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    indices = np.concatenate(cols).astype(np.int32)
    data = rng.integers(1, 60000, len(indices)).astype(np.uint16)
    cell = np.array([0, 0, 0, 0, 1], np.int32)
    umi = np.array([2, 2, 2, 2, 2], np.int32)
    rep, stats = _check(indptr, indices, data, k, cell, umi)
    assert stats.tolist() == [5, 2, 3, 2] and rep[0] == rep[1] and rep[2] == rep[3] and rep[4] == 4


def test_rows_without_entries(gpu_device):
    rng = np.random.default_rng(7)
    n, k = 1000, 20
    lens = rng.integers(0, 4, n)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    indices = np.concatenate([rng.permutation(k)[:ln] for ln in lens]).astype(np.int32)
    data = rng.integers(1, 30, int(indptr[-1])).astype(np.uint16)
    cell = rng.integers(-1, 4, n).astype(np.int32)
    umi = rng.integers(-1, 6, n).astype(np.int32)
    rep, stats = _check(indptr, indices, data, k, cell, umi, 4, 6)
    assert (lens == 0).sum() > 100 and np.all(rep[lens == 0] == np.flatnonzero(lens == 0)) and stats[3] > 100
    # a matrix without any entry
    rep, stats = _check(np.zeros(6, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16), 4, np.zeros(5, np.int32), np.zeros(5, np.int32))
    assert rep.tolist() == [0, 1, 2, 3, 4] and stats.tolist() == [5, 1, 5, 0]


def test_no_rows(gpu_device):
    rep, stats = _device(np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.uint16), 5, np.zeros(0, np.int32), np.zeros(0, np.int32), 3, 3)
    assert rep.shape == (0,) and stats.tolist() == [0, 0, 0, 0]


def test_no_row_in_any_class_and_every_row_a_class(gpu_device):
    (indptr, indices, data, cell, umi, k), _ = _random(1)
    n = len(cell)
    rep, stats = _check(indptr, indices, data, k, np.full(n, -1, np.int32), umi, 12, 40)          # every cell -1
    assert np.array_equal(rep, np.arange(n)) and stats.tolist() == [0, 0, 0, 0]
    rep, stats = _check(indptr, indices, data, k, cell, np.full(n, -1, np.int32), 12, 0)           # every UMI -1, n_umis = 0
    assert np.array_equal(rep, np.arange(n)) and stats.tolist() == [0, 0, 0, 0]
    own = np.arange(n, dtype=np.int32)
    rep, stats = _check(indptr, indices, data, k, np.zeros(n, np.int32), own, 1, n)                # every row a class of its own
    assert np.array_equal(rep, own) and stats.tolist() == [n, n, n, 0]


def test_one_cell_one_umi(gpu_device):
    (indptr, indices, data, cell, umi, k), _ = _random(2)
    rep, stats = _check(indptr, indices, data, k, np.minimum(cell, 0), np.minimum(umi, 0), 1, 1)
    assert stats[1] == 1 and stats[3] > 2000


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_same_result_whatever_the_handle_holds_and_the_state_is_untouched(gpu_device):
    from telescope_amd.likelihood import TelescopeLikelihood
    (indptr, indices, data, cell, umi, k), (want_rep, want_stats) = _random(3)
    raw = _canonical(indptr, indices, data, k)

    def same(eng):
        rep, stats = eng.umi_dedup(cell, umi, 12, 40)
        return np.array_equal(rep, want_rep) and np.array_equal(stats, want_stats)

    eng = _engine(indptr, indices, data, k)                  # before tsem_set_lut: only the matrix is there
    assert same(eng)
    eng.close()

    def fitted(call, options):
        """a complete fit, then (`call`) the dedup, then the group map's counts and the per-cell fits"""
        tl = TelescopeLikelihood(raw, Opts(max_iter=30), engine_options=options)
        tl.em()
        before = (tl._eng.get_params(1), tl._eng.get_params(0), tl._eng.final_lnl())
        if call:
            assert same(tl._eng)
            after = (tl._eng.get_params(1), tl._eng.get_params(0), tl._eng.final_lnl())
            for a, b in zip(before[:2], after[:2]):
                assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])
            assert before[2] == after[2]
        counts = tl.reassign_cell_counts('exclude', np.maximum(cell, -1), 12)
        if call:
            assert same(tl._eng)                             # with a group map, its grouping and counts resident
            again = tl.reassign_cell_counts('exclude', np.maximum(cell, -1), 12)
            assert _same_bits(counts.data, again.data) and _same_bits(counts.indices, again.indices)
        fits = tl.em_cells(cell, 12)
        if call:
            assert same(tl._eng)                             # after the per-cell fits
        out = dict(pi=tl.pi.copy(), theta=tl.theta.copy(), lnl=tl.lnl, counts=counts, fits=fits,
                   cell_counts=tl.reassign_cell_counts('average', cell, 12))
        tl._eng.close()
        return out

    for options in ({'reproducible': 1}, {'reproducible': 1, 'drop_csr_indices': 1}):
        a, b = fitted(True, options), fitted(False, options)     # b: a handle that never made the call
        assert _same_bits(a['pi'], b['pi']) and _same_bits(a['theta'], b['theta']) and a['lnl'] == b['lnl']
        for key in ('counts', 'cell_counts'):
            assert _same_bits(a[key].indptr, b[key].indptr) and _same_bits(a[key].indices, b[key].indices) and _same_bits(a[key].data, b[key].data)
        for name in ('col_ptr', 'cols', 'pi', 'theta', 'n_iter', 'converged', 'lnl'):
            assert _same_bits(getattr(a['fits'], name), getattr(b['fits'], name)), name


def _refused(eng, cell, umi, n_cells, n_umis, rep, stats, word):
    from telescope_amd import _lib
    rc = eng._L.tsem_umi_dedup(eng._h, _lib.ptr(cell), _lib.ptr(umi), n_cells, n_umis, _lib.ptr(rep), _lib.ptr(stats))
    msg = eng._L.tsem_last_error(eng._h).decode()
    assert rc == _lib.ERR_ARG and 'tsem_umi_dedup' in msg and word in msg, (rc, msg)


def test_refusals(gpu_device):
    from telescope_amd import _lib
    (indptr, indices, data, cell, umi, k), (want_rep, want_stats) = _random(1)
    n = len(cell)
    rep, stats = np.empty(n, np.int32), np.zeros(4, np.int64)
    eng = _lib.Engine(0)
    _refused(eng, cell, umi, 12, 40, rep, stats, 'no matrix')
    eng.close()
    eng = _engine(indptr, indices, data, k)
    for bad_cell, bad_umi in ((12, None), (-2, None), (None, 40), (None, -2)):
        c, u = cell.copy(), umi.copy()
        if bad_cell is not None:
            c[n - 1] = bad_cell
        if bad_umi is not None:
            u[0] = bad_umi
        _refused(eng, c, u, 12, 40, rep, stats, 'outside')
    _refused(eng, None, umi, 12, 40, rep, stats, 'NULL')
    _refused(eng, cell, None, 12, 40, rep, stats, 'NULL')
    _refused(eng, cell, umi, 12, 40, None, stats, 'NULL')
    group = _lib.LocalGroup(0, 1)                            # the in-process transport: a communicator attached
    comm = group.comm(0)
    eng.comm_attach(comm.handle)
    _refused(eng, cell, umi, 12, 40, rep, stats, 'row-sharded')
    eng.comm_attach(None)
    got_rep, got_stats = eng.umi_dedup(cell, umi, 12, 40)    # the refusals left a handle that works
    assert np.array_equal(got_rep, want_rep) and np.array_equal(got_stats, want_stats)
    eng.close()
    comm.close()
    group.close()


# ---- end to end: `sc assign --umi_tag` / `sc resume` against plain runs of the collapsed matrix ---------------------------------------
SIX = ['TE_counts_%s.tsv' % m for m in ('conf', 'all', 'unique', 'exclude', 'choose', 'average')]


def _cli(argv, outdir, quiet=True):
    import subprocess
    import sys
    r = subprocess.run([sys.executable, '-m', 'telescope_amd'] + argv + ['--outdir', str(outdir)] + (['--quiet'] if quiet else []), cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _same_files(a, b, names):
    for name in names:
        fa, fb = os.path.join(str(a), 'telescope-' + name), os.path.join(str(b), 'telescope-' + name)
        assert open(fa, 'rb').read() == open(fb, 'rb').read(), name


def _collapsed_checkpoint(checkpoint, path):
    """the checkpoint of the collapsed run, by the host definition: raw[keep], cell_of_row[keep], no UMIs"""
    from telescope_amd.run_container import scTelescope
    ts = scTelescope.load(checkpoint)
    raw = ts.raw_scores.tocsr()
    rep, stats = dedup_plain(raw.indptr, raw.indices, raw.data, ts.cell_of_row, ts.umi_of_row)
    keep = rep == np.arange(len(rep))
    names = sorted(ts.read_index, key=ts.read_index.get)
    ts.raw_scores = raw[np.flatnonzero(keep)]
    ts.shape = ts.raw_scores.shape
    ts.cell_of_row = ts.cell_of_row[keep]
    ts.read_index = {nm: i for i, nm in enumerate(n for n, k in zip(names, keep) if k)}
    ts.umi_of_row = ts.umis = None
    ts.save(path)
    return keep, stats


@pytest.fixture(scope='module')
def mixed_run(gpu_device, tmp_path_factory):
    out = tmp_path_factory.mktemp('umi_mixed')
    log = _cli(['sc', 'assign', os.path.join(GOLD, 'sc_mixed.bam'), os.path.join(GOLD, 'sc_mixed.gtf'), '--umi_tag', 'UB',
                '--use_every_reassign_mode'], out, quiet=False)
    return out, log


def test_end_to_end_sc_mixed_keeps_23_of_91(mixed_run, tmp_path):
    from telescope_amd.run_container import scTelescope
    out, log = mixed_run
    ck = scTelescope.load(str(out / 'telescope-checkpoint.npz'))
    assert ck.shape[0] == 91 and ck.umis == ['UMI1'] and np.all(ck.umi_of_row == 0)      # the uncollapsed run, with its UMIs
    keep, stats = _collapsed_checkpoint(str(out / 'telescope-checkpoint.npz'), str(tmp_path / 'collapsed'))
    assert int(keep.sum()) == 23
    assert 'UMI duplicates: collapsed 68 of 91 fragments (%d barcode-UMI classes, %d molecules)' % (stats[1], stats[2]) in log
    assert '    umi_tag:                      UB' in log
    _cli(['sc', 'resume', str(tmp_path / 'collapsed.npz'), '--use_every_reassign_mode'], tmp_path / 'plain')
    _same_files(out, tmp_path / 'plain', SIX + ['run_stats.tsv'])
    assert not os.path.exists(str(tmp_path / 'plain' / 'telescope-umi_stats.tsv'))
    lines = open(str(out / 'telescope-umi_stats.tsv')).read().split('\n')[1:-1]
    assert len(lines) == len(ck.barcodes) and sum(int(ln.split('\t')[3]) for ln in lines) == int((keep & (ck.cell_of_row >= 0)).sum())


def test_sc_resume_of_the_checkpoint_gives_the_same_files(mixed_run, tmp_path):
    out, _ = mixed_run
    log = _cli(['sc', 'resume', str(out / 'telescope-checkpoint.npz'), '--use_every_reassign_mode'], tmp_path, quiet=False)
    assert 'UMI duplicates: collapsed 68 of 91 fragments' in log and 'umi_tag' not in log
    _same_files(out, tmp_path, SIX + ['run_stats.tsv', 'umi_stats.tsv'])


def test_end_to_end_individual_pooling_on_the_umi_fixture(gpu_device, tmp_path):
    exp = np.load(os.path.join(GOLD, 'sc_umi_expected.npz'), allow_pickle=False)
    _cli(['sc', 'assign', os.path.join(GOLD, 'sc_umi.bam'), os.path.join(GOLD, 'sc_umi.gtf'), '--umi_tag', 'UB', '--pooling_mode', 'individual'],
         tmp_path / 'a')
    keep, stats = _collapsed_checkpoint(str(tmp_path / 'a' / 'telescope-checkpoint.npz'), str(tmp_path / 'collapsed'))
    assert np.array_equal(keep, exp['rep_of_row'] == np.arange(len(keep))) and np.array_equal(stats, exp['stats'])
    _cli(['sc', 'resume', str(tmp_path / 'collapsed.npz'), '--pooling_mode', 'individual'], tmp_path / 'plain')
    _same_files(tmp_path / 'a', tmp_path / 'plain', ['TE_counts.tsv', 'run_stats.tsv', 'cell_stats.tsv'])
    kept = [int(ln.split('\t')[3]) for ln in open(str(tmp_path / 'a' / 'telescope-umi_stats.tsv')).read().split('\n')[1:-1]]
    cor = exp['cell_of_row']
    assert kept == np.bincount(cor[keep & (cor >= 0)], minlength=len(exp['barcodes'])).tolist()


def test_ignore_umi_gives_the_files_of_a_run_without_umi_tag(gpu_device, tmp_path):
    from telescope_amd.run_container import scTelescope
    bam, gtf = os.path.join(GOLD, 'sc_umi.bam'), os.path.join(GOLD, 'sc_umi.gtf')
    log = _cli(['sc', 'assign', bam, gtf, '--umi_tag', 'UB', '--ignore_umi', '--use_every_reassign_mode'], tmp_path / 'i', quiet=False)
    _cli(['sc', 'assign', bam, gtf, '--use_every_reassign_mode'], tmp_path / 'p')
    _same_files(tmp_path / 'i', tmp_path / 'p', SIX + ['run_stats.tsv'])
    assert 'UMI duplicates' not in log and not os.path.exists(str(tmp_path / 'i' / 'telescope-umi_stats.tsv'))
    ck = scTelescope.load(str(tmp_path / 'i' / 'telescope-checkpoint.npz'))                # the UMIs are stored all the same
    assert ck.umi_of_row is not None and len(ck.umis) == 29
    assert 'umi' not in ' '.join(np.load(str(tmp_path / 'p' / 'telescope-checkpoint.npz')).files)
