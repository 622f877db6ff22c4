"""UMI collapsing on the host: the loader's `umi_tag`, the checkpoint keys, `collapse_umis` bookkeeping, the `sc` options, the
umi_stats writer and the argument checks of `likelihood.umi_dedup` — nothing here needs a device (the device call is stubbed)."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

from _umi_reference import dedup_plain
from conftest import GOLD

BAM, GTF = os.path.join(GOLD, 'sc_umi.bam'), os.path.join(GOLD, 'sc_umi.gtf')
MIXED_BAM, MIXED_GTF = os.path.join(GOLD, 'sc_mixed.bam'), os.path.join(GOLD, 'sc_mixed.gtf')


def _load(bam=BAM, gtf=GTF, **kw):
    from telescope_amd import loader
    return loader.load_alignment(bam, loader.Annotation(gtf), **kw)


def test_loader_reads_the_umis_of_the_fixture():
    exp = np.load(os.path.join(GOLD, 'sc_umi_expected.npz'), allow_pickle=False)
    out = _load(barcode_tag='CB', umi_tag='UB')
    raw = out['raw_scores'].tocsr()
    assert tuple(exp['shape']) == raw.shape
    assert np.array_equal(raw.indptr, exp['indptr']) and np.array_equal(raw.indices, exp['indices']) and np.array_equal(raw.data, exp['data'])
    assert out['cell_of_row'].dtype == np.int32 and np.array_equal(out['cell_of_row'], exp['cell_of_row'])
    assert out['umi_of_row'].dtype == np.int32 and np.array_equal(out['umi_of_row'], exp['umi_of_row'])
    assert out['barcodes'] == list(exp['barcodes']) and out['umis'] == list(exp['umis'])
    uor = out['umi_of_row']
    assert (uor == -1).any() and (out['cell_of_row'][uor >= 0] == -1).any()      # without UB; with UB and without CB
    seen = uor[uor >= 0]
    first = [int(u) for i, u in enumerate(seen) if u not in seen[:i]]
    assert first == list(range(len(out['umis'])))                # numbered by first appearance among the rows
    assert 'GHOST' not in out['umis']                            # the UMI of fragments that are no rows
    # the recorded representatives are those of the definition on the recorded matrix
    rep, stats = dedup_plain(raw.indptr, raw.indices, raw.data, out['cell_of_row'], uor)
    assert np.array_equal(rep, exp['rep_of_row']) and np.array_equal(stats, exp['stats'])
    row = out['read_index']
    assert rep[row['chainA']] == rep[row['chainC']] == row['chainB']              # the chain of three
    assert rep[row['splitA']] != rep[row['splitB']] and uor[row['splitA']] == uor[row['splitB']]   # one class, two components
    assert rep[row['tieB']] == rep[row['tieC']] == row['tieA']                    # the tie: the smallest row
    assert uor[row['shareA']] == uor[row['shareB']] and rep[row['shareA']] != rep[row['shareB']]   # one UMI, two cells


def test_loader_without_umi_tag_is_unchanged():
    a, b = _load(barcode_tag='CB'), _load(barcode_tag='CB', umi_tag='UB')
    assert sorted(a) == sorted(set(b) - {'umi_of_row', 'umis'})
    assert (a['raw_scores'] != b['raw_scores']).nnz == 0 and a['run_info'] == b['run_info'] and a['read_index'] == b['read_index']
    assert np.array_equal(a['cell_of_row'], b['cell_of_row']) and a['barcodes'] == b['barcodes']
    c = _load(umi_tag='UB')                                      # UMIs without barcodes
    assert 'cell_of_row' not in c and np.array_equal(c['umi_of_row'], b['umi_of_row'])
    from telescope_amd import loader
    refs, recs = loader.read_bam(BAM)
    assert all(s.umi is None and s.bc is None for s in recs)


def test_sc_mixed_has_one_umi_for_all_rows():
    out = _load(MIXED_BAM, MIXED_GTF, barcode_tag='CB', umi_tag='UB')
    assert out['raw_scores'].shape[0] == 91 and out['umis'] == ['UMI1'] and np.all(out['umi_of_row'] == 0)
    raw = out['raw_scores'].tocsr()
    rep, _ = dedup_plain(raw.indptr, raw.indices, raw.data, out['cell_of_row'], out['umi_of_row'])
    assert int(np.sum(rep == np.arange(91))) == 23


def _container(umi_tag='UB'):
    from telescope_amd import loader
    from telescope_amd.run_container import scTelescope

    class O(object):
        samfile, gtffile, no_feature_key, overlap_mode, overlap_threshold, stranded_mode, barcode_tag = \
            BAM, GTF, '__no_feature', 'threshold', 0.2, 'None', 'CB'
        outdir, exp_tag = '.', 'telescope'
    O.umi_tag = umi_tag
    ts = scTelescope(O())
    ts.run_info['version'] = 'v'
    ts.load_alignment(loader.Annotation(GTF))
    return ts


def test_checkpoint_round_trips(tmp_path):
    from telescope_amd.run_container import scTelescope
    with_umi, without = _container(), _container(None)
    assert without.umi_of_row is None and without.umis is None
    with_umi.save(str(tmp_path / 'u'))
    without.save(str(tmp_path / 'p'))
    zu, zp = np.load(str(tmp_path / 'u.npz')), np.load(str(tmp_path / 'p.npz'))
    today = {'_run_info', '_flen_list', '_feat_list', '_read_list', '_shape', '_raw_scores_data', '_raw_scores_indices',
             '_raw_scores_indptr', '_raw_scores_shape', '_barcode_list', '_read_barcode'}
    assert set(zp.files) == today and set(zu.files) == today | {'_umi_list', '_read_umi'}
    for k in zp.files:
        assert zu[k].dtype == zp[k].dtype and zu[k].tobytes() == zp[k].tobytes(), k
    assert zu['_read_umi'].dtype == np.int32
    back = scTelescope.load(str(tmp_path / 'u.npz'))
    assert back.umis == with_umi.umis and np.array_equal(back.umi_of_row, with_umi.umi_of_row) and back.umi_of_row.dtype == np.int32
    assert np.array_equal(back.cell_of_row, with_umi.cell_of_row) and (back.raw_scores != with_umi.raw_scores).nnz == 0
    plain = scTelescope.load(str(tmp_path / 'p.npz'))
    assert plain.umi_of_row is None and plain.umis is None


@pytest.mark.parametrize('what', ['short', 'too large', 'below -1', 'list only'])
def test_corrupt_read_umi_is_refused(tmp_path, what):
    from telescope_amd.run_container import scTelescope
    ts = _container()
    ts.save(str(tmp_path / 'u'))
    z = dict(np.load(str(tmp_path / 'u.npz')))
    if what == 'short':
        z['_read_umi'] = z['_read_umi'][:-1]
    elif what == 'too large':
        z['_read_umi'][3] = len(z['_umi_list'])
    elif what == 'below -1':
        z['_read_umi'][3] = -2
    else:
        del z['_read_umi']
    np.savez(str(tmp_path / 'bad'), **z)
    with pytest.raises(ValueError, match='_read_umi'):
        scTelescope.load(str(tmp_path / 'bad.npz'))
    from telescope_amd import cli
    with pytest.raises(SystemExit, match='_read_umi'):
        cli.main(['sc', 'resume', str(tmp_path / 'bad.npz'), '--outdir', str(tmp_path), '--quiet'])


def test_collapse_umis_bookkeeping_and_the_stats_file(tmp_path, monkeypatch):
    from telescope_amd import likelihood
    ts = _container()
    n, names = ts.shape[0], sorted(ts.read_index, key=ts.read_index.get)
    raw0, cor0, uor0 = ts.raw_scores.copy(), ts.cell_of_row.copy(), ts.umi_of_row.copy()
    rep, stats = dedup_plain(raw0.indptr, raw0.indices, raw0.data, cor0, uor0)
    seen = {}

    def stub(raw_scores, cell_of_row, umi_of_row, device=0, n_cells=None, n_umis=None):
        seen.update(device=device, n_cells=n_cells, n_umis=n_umis, shape=raw_scores.shape)
        assert np.array_equal(cell_of_row, cor0) and np.array_equal(umi_of_row, uor0)
        return likelihood.UmiDedup(rep, stats, cell_of_row)
    monkeypatch.setattr(likelihood, 'umi_dedup', stub)
    d = ts.collapse_umis(device=3)
    assert seen == dict(device=3, n_cells=len(ts.barcodes), n_umis=len(ts.umis), shape=(n, raw0.shape[1]))
    keep = rep == np.arange(n)
    assert d is ts.umi_dedup and np.array_equal(d.keep, keep) and d.n_dropped == int((~keep).sum()) == stats[3]
    assert (d.n_class_rows, d.n_classes, d.n_components) == tuple(int(x) for x in stats[:3])
    assert ts.shape == (int(keep.sum()), raw0.shape[1]) == ts.raw_scores.shape
    assert (ts.raw_scores != raw0[np.flatnonzero(keep)]).nnz == 0 and ts.raw_scores.dtype == raw0.dtype
    assert np.array_equal(ts.cell_of_row, cor0[keep]) and np.array_equal(ts.umi_of_row, uor0[keep])
    assert ts.cell_of_row.dtype == np.int32 and ts.umi_of_row.dtype == np.int32
    assert sorted(ts.read_index, key=ts.read_index.get) == [nm for nm, k in zip(names, keep) if k]
    assert sorted(ts.read_index.values()) == list(range(int(keep.sum())))
    ts.write_umi_stats(str(tmp_path / 'x-umi_stats.tsv'))
    lines = open(str(tmp_path / 'x-umi_stats.tsv')).read().split('\n')
    assert lines[0] == 'barcode\tfragments\twith_umi\tkept' and lines[-1] == '' and len(lines) == len(ts.barcodes) + 2
    for c, b in enumerate(ts.barcodes):
        want = [b, int((cor0 == c).sum()), int(((cor0 == c) & (uor0 >= 0)).sum()), int((keep & (cor0 == c)).sum())]
        assert lines[1 + c].split('\t') == [str(x) for x in want]
    assert np.array_equal(d.kept_per_cell(len(ts.barcodes)), np.bincount(cor0[keep & (cor0 >= 0)], minlength=len(ts.barcodes)))
    with pytest.raises(ValueError, match='no UMIs'):
        _container(None).collapse_umis()
    with pytest.raises(ValueError, match='not collapsed'):
        _container().write_umi_stats(str(tmp_path / 'y'))


def test_the_options_exist_on_the_sc_commands_only():
    from telescope_amd.cli import ResumeOptions, build_parser
    ap = build_parser()
    a = vars(ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf']))
    assert a['umi_tag'] is None and a['ignore_umi'] is False
    a = ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf', '--umi_tag', 'UB', '--ignore_umi'])
    assert a.umi_tag == 'UB' and a.ignore_umi is True
    assert '    umi_tag:                      UB' in str(ResumeOptions(a)).split('\n')
    assert 'umi_tag' not in str(ResumeOptions(ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf'])))
    r = vars(ap.parse_args(['sc', 'resume', 'c.npz']))
    assert 'umi_tag' not in r and r['ignore_umi'] is False
    assert ap.parse_args(['sc', 'resume', 'c.npz', '--ignore_umi']).ignore_umi is True
    for argv in (['assign', 'x.bam', 'y.gtf'], ['resume', 'c.npz']):
        ns = vars(ap.parse_args(argv))
        assert 'umi_tag' not in ns and 'ignore_umi' not in ns
        for opt in (['--umi_tag', 'UB'], ['--ignore_umi']):
            with pytest.raises(SystemExit):
                ap.parse_args(argv + opt)


def test_umi_tag_with_updated_sam_is_refused_before_any_file_is_opened(tmp_path, monkeypatch):
    import builtins
    import gzip
    from telescope_amd import cli

    def no_open(*a, **kw):
        raise AssertionError('a file was opened: %r' % (a[:1],))
    monkeypatch.setattr(gzip, 'open', no_open)
    monkeypatch.setattr(builtins, 'open', no_open)
    out = tmp_path / 'never'
    with pytest.raises(SystemExit, match='--umi_tag with --updated_sam'):
        cli.main(['sc', 'assign', str(tmp_path / 'missing.bam'), str(tmp_path / 'missing.gtf'), '--umi_tag', 'UB', '--updated_sam',
                  '--outdir', str(out)])
    monkeypatch.undo()
    assert not out.exists()


def test_argument_checks_need_no_device(monkeypatch):
    from telescope_amd import likelihood

    def no_engine(*a, **kw):
        raise AssertionError('the device was asked for')
    monkeypatch.setattr(likelihood, 'Engine', no_engine)
    raw = sp.csr_matrix(np.array([[3, 0], [0, 4], [5, 5]], np.uint16))
    ok = np.zeros(3, np.int32)
    for cell, umi, kw, word in (
            (ok[:2], ok, {}, 'cell_of_row'), (ok, ok[:2], {}, 'umi_of_row'), (ok.astype(float), ok, {}, 'cell_of_row'),
            (np.array([0, -2, 0]), ok, {}, 'cell_of_row'), (ok, np.array([0, 0, -5]), {}, 'umi_of_row'),
            (np.array([0, 1, 2]), ok, {'n_cells': 2}, 'cell_of_row'), (ok, np.array([0, 7, 0]), {'n_umis': 7}, 'umi_of_row'),
            (np.array([0, 2 ** 31, 0]), ok, {}, 'cell_of_row'), (ok, ok, {'n_umis': -1}, 'umi_of_row')):
        with pytest.raises(ValueError, match=word):
            likelihood.umi_dedup(raw, cell, umi, **kw)
    c, u, n_cells, n_umis = likelihood.check_umi_args(3, np.array([0, 4, -1], np.int64), [2, -1, 0])
    assert c.dtype == np.int32 and u.dtype == np.int32 and (n_cells, n_umis) == (5, 3)     # taken from the data
    assert likelihood.check_umi_args(0, np.zeros(0, np.int32), np.zeros(0, np.int32))[2:] == (0, 0)
    assert likelihood.check_umi_args(3, ok - 1, ok - 1)[2:] == (0, 0)
    with pytest.raises(AssertionError, match='the device was asked for'):                 # good arguments go on to the device
        likelihood.umi_dedup(raw, ok, ok)
    d = likelihood.UmiDedup(np.array([1, 1, 2], np.int32), [2, 1, 1, 1], np.array([0, 0, -1], np.int32))
    assert d.keep.tolist() == [False, True, True] and d.kept_per_cell(2).tolist() == [1, 0] and d.n_dropped == 1
