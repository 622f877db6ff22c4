"""`sc --pooling_mode celltype` without a device: the cell type file and everything the command line refuses, the type of every
fragment, the celltype_stats.tsv writer, and what tests/test_gpu_group_em.py relies on — no iteration count it compares hinges on a
rounding, and the ties of the end-to-end fixture are exact on both sides."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import _cell_em_reference as R
import _group_em_reference as GR

GOLDEN = GR.GOLDEN
BAM, GTF = os.path.join(GOLDEN, 'sc_mixed.bam'), os.path.join(GOLDEN, 'sc_mixed.gtf')


@pytest.fixture(autouse=True)
def _no_device(monkeypatch):
    monkeypatch.setenv('TSEM_NO_WARM', '1')                  # (a refused run must not bring a device up behind the test)


def _tsv(tmp_path, text, name='types.tsv'):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


# ---- the file ------------------------------------------------------------------------------------------------------------------
def test_tsv_is_read_as_documented(tmp_path):
    from telescope_amd.run_container import read_celltype_tsv
    got = read_celltype_tsv(_tsv(tmp_path, '# a comment\nAAAC\tT cell\n\nTTTG\tB\nCCCA\tT cell\nAAAC\tT cell\n'))
    assert list(got.items()) == [('AAAC', 'T cell'), ('TTTG', 'B'), ('CCCA', 'T cell')]
    got = read_celltype_tsv(GR.E2E_TSV)
    assert sorted(set(got.values())) == list(GR.E2E_TYPES) and GR.E2E_OMITTED not in got and 'NNNN' in got


@pytest.mark.parametrize('text, word', [('AAAC T\n', 'expected barcode<TAB>celltype'), ('AAAC\tT\textra\n', 'expected barcode<TAB>celltype'),
                                        ('AAAC\t\n', 'expected barcode<TAB>celltype'), ('AAAC\tT\nAAAC\tB\n', 'two cell types')])
def test_tsv_errors(tmp_path, text, word):
    from telescope_amd.run_container import read_celltype_tsv
    with pytest.raises(ValueError) as e:
        read_celltype_tsv(_tsv(tmp_path, text))
    assert word in str(e.value)
    with pytest.raises(ValueError):
        read_celltype_tsv(str(tmp_path / 'missing.tsv'))


def test_types_are_numbered_by_sorted_name_and_unlisted_barcodes_have_none():
    from telescope_amd.run_container import celltype_map, compose_type_of_row
    names, toc = celltype_map(['b0', 'b1', 'b2', 'b3'], {'b3': 'zeta', 'b0': 'alpha', 'elsewhere': 'beta', 'b1': 'zeta'})
    assert names == ['alpha', 'beta', 'zeta'] and toc.tolist() == [0, 2, -1, 2] and toc.dtype == np.int32
    cor = np.array([0, 1, 2, 3, -1, 2, 0], np.int32)
    tor = compose_type_of_row(cor, toc)
    assert tor.tolist() == [0, 2, -1, 2, -1, -1, 0] and tor.dtype == np.int32
    with pytest.raises(ValueError):
        celltype_map(['b0', 'b1'], {'elsewhere': 'beta'})
    assert compose_type_of_row(np.zeros(0, np.int32), toc).shape == (0,)


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_parser_takes_the_mode_and_the_file_on_both_sc_subcommands():
    from telescope_amd import cli
    ap = cli.build_parser()
    a = ap.parse_args(['sc', 'assign', 'x.bam', 'y.gtf', '--pooling_mode', 'celltype', '--celltype_tsv', 't.tsv'])
    assert a.pooling_mode == 'celltype' and a.celltype_tsv == 't.tsv'
    r = ap.parse_args(['sc', 'resume', 'c.npz', '--pooling_mode', 'celltype', '--celltype_tsv', 't.tsv'])
    assert r.pooling_mode == 'celltype' and r.celltype_tsv == 't.tsv'
    assert ap.parse_args(['sc', 'resume', 'c.npz']).celltype_tsv is None
    for argv in (['sc', 'assign', 'x.bam', 'y.gtf'], ['sc', 'resume', 'c.npz']):   # the mode without its file: refused where it is parsed
        with pytest.raises(SystemExit) as e:
            ap.parse_args(argv + ['--pooling_mode', 'celltype'])
        assert 'needs --celltype_tsv' in str(e.value.code) and ' '.join(argv[:2]) in str(e.value.code)
    for argv in (['assign', 'x.bam', 'y.gtf'], ['resume', 'c.npz']):
        with pytest.raises(SystemExit):
            ap.parse_args(argv + ['--celltype_tsv', 't.tsv'])
    import argparse
    for p in (cli._sc_args(cli._assign_args(argparse.ArgumentParser()), True), cli._sc_args(cli._resume_args(argparse.ArgumentParser()), False)):
        group = [g for g in p._action_groups if g.title == 'Input Options'][0]
        assert any('--celltype_tsv' in a.option_strings for a in group._group_actions)
    shown = str(cli.ResumeOptions(ap.parse_args(['sc', 'resume', 'c.npz', '--pooling_mode', 'celltype', '--celltype_tsv', 't.tsv'])))
    assert shown.splitlines()[-1].split() == ['celltype_tsv:', 't.tsv']
    assert 'celltype_tsv' not in str(cli.ResumeOptions(ap.parse_args(['sc', 'resume', 'c.npz'])))


def _refused(argv, tmp_path, *words):
    from telescope_amd import cli
    out = tmp_path / 'out'
    with pytest.raises(SystemExit) as e:
        cli.main(argv + ['--quiet', '--outdir', str(out)])
    assert isinstance(e.value.code, str), e.value.code       # (a message, not argparse's exit status)
    for w in words:
        assert w in str(e.value), (w, str(e.value))
    assert not out.exists()                                  # nothing written


def _ckpt(tmp_path):
    """a single-cell checkpoint of the fixture, written on the host"""
    ts = GR.load_sc_mixed()
    path = str(tmp_path / 'sc-checkpoint.npz')
    ts.save(path)
    return path


@pytest.mark.parametrize('command', ['assign', 'resume'])
def test_every_refusal(tmp_path, command):
    """Each refused before the alignments, the checkpoint or the device are touched: the input files named here do not exist."""
    head = ['sc', 'assign', str(tmp_path / 'no.bam'), str(tmp_path / 'no.gtf')] if command == 'assign' else ['sc', 'resume', str(tmp_path / 'no.npz')]
    good = _tsv(tmp_path, 'AAAC\tT\n')
    _refused(head + ['--pooling_mode', 'celltype'], tmp_path, 'needs --celltype_tsv')
    _refused(head + ['--pooling_mode', 'celltype', '--celltype_tsv', str(tmp_path / 'missing.tsv')], tmp_path, 'cannot read')
    _refused(head + ['--pooling_mode', 'celltype', '--celltype_tsv', _tsv(tmp_path, 'AAAC T\n', 'a.tsv')], tmp_path, 'line 1')
    _refused(head + ['--pooling_mode', 'celltype', '--celltype_tsv', _tsv(tmp_path, 'AAAC\tT\n#x\nAAAC\tB\n', 'b.tsv')], tmp_path, 'line 3', 'two cell types')
    for mode in ('pseudobulk', 'individual'):
        _refused(head + ['--pooling_mode', mode, '--celltype_tsv', good], tmp_path, '--celltype_tsv', mode)
    _refused(head + ['--celltype_tsv', good], tmp_path, '--celltype_tsv', 'pseudobulk')
    if command == 'assign':
        _refused(head + ['--pooling_mode', 'celltype', '--celltype_tsv', good, '--updated_sam'], tmp_path,
                 '--pooling_mode celltype with --updated_sam is not supported', 'pooled posteriors')


def test_a_file_that_names_no_barcode_of_the_run_is_refused(tmp_path):
    """... once the barcodes are known: after the alignments are read (assign; before the checkpoint is written) or the checkpoint is
    loaded (resume), and before the model is built."""
    strangers = _tsv(tmp_path, 'NNNN\tT\nMMMM\tB\n')
    _refused(['sc', 'assign', BAM, GTF, '--pooling_mode', 'celltype', '--celltype_tsv', strangers], tmp_path, 'names none of the 5 barcodes')
    _refused(['sc', 'resume', _ckpt(tmp_path), '--pooling_mode', 'celltype', '--celltype_tsv', strangers], tmp_path, 'names none of the 5 barcodes')


def test_skip_em_with_a_good_file_writes_the_checkpoint_only(tmp_path):
    from telescope_amd import cli
    out = tmp_path / 'o'
    assert cli.main(['sc', 'assign', BAM, GTF, '--pooling_mode', 'celltype', '--celltype_tsv', GR.E2E_TSV, '--skip_em', '--quiet', '--outdir', str(out)]) == 0
    assert os.listdir(str(out)) == ['telescope-checkpoint.npz']


# ---- the stats file ------------------------------------------------------------------------------------------------------------
def test_celltype_stats_writer(tmp_path):
    from telescope_amd.likelihood import CellFits
    from telescope_amd.run_container import scTelescope
    ts = scTelescope()
    ts.barcodes = ['b0', 'b1', 'b2', 'b3']
    ts.cell_of_row = np.array([0, 1, 2, 3, -1, 2, 0, 1], np.int32)
    ts.set_celltypes({'b3': 'zeta', 'b0': 'al\tpha', 'gone': 'beta', 'b1': 'zeta'})     # b2: no type; beta: no cell of the run

    class TL(object):
        Y = np.array([[1], [0], [1], [1], [1], [1], [0], [1]])
    v = np.arange(5, dtype=float)
    fits = CellFits(6, [0, 2, 2, 5], np.array([1, 4, 0, 2, 5], np.int32), v, v, v, v, np.zeros((3, 4)), [3, 0, 100], [1, 0, 0],
                    [-1.5, np.nan, 0.1 + 0.2])
    path = str(tmp_path / 'x-celltype_stats.tsv')
    ts.write_celltype_stats(TL(), fits, path)
    lines = open(path).read().splitlines()
    assert lines[0].split('\t') == ['celltype', 'cells', 'fragments', 'ambiguous', 'columns', 'iterations', 'converged', 'lnl']
    assert lines[1] == '"al\tpha"\t1\t2\t1\t2\t3\tTrue\t-1.5'
    assert lines[2] == 'beta\t0\t0\t0\t0\t0\tFalse\tnan'
    assert lines[3] == 'zeta\t2\t3\t2\t3\t100\tFalse\t0.30000000000000004'
    assert len(lines) == 4


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------------------
def test_the_tier_and_chunk_cases_are_what_they_say():
    raw, cor, n = GR.tier_case()
    L, W, T = GR.SP_LANE, GR.SP_WAVE, GR.SP_T
    assert [GR.column_counts(raw, cor, c) for c in range(n)] == [
        [L, L, L + 1, L + 1], [64, 64, 65, 65], [192, 192, 193, 193], [W, W + 1], [T * 17, T * 17 + 1], [1, 2, 2]]
    raw, cor, n = GR.chunk_case()
    assert np.bincount(cor[cor >= 0]).tolist() == [GR.SP_ROWS, GR.SP_ROWS + 1, 1]
    assert raw[np.flatnonzero(cor == 2)].nnz > 1             # (spread when forced: more than one stored entry)
    assert GR.LOOK_ITERS == (1, 7, 8, 9)


def test_no_compared_iteration_count_hinges_on_a_rounding():
    """The spread class adds in another order than the one-workgroup classes and the oracle: every stop test of every case whose
    iteration counts the GPU tests compare stays 1e-6 (relative) clear of epsilon."""
    n = 0
    for label, ref in GR.iteration_count_cases():
        m = R.stop_margin(ref)
        assert m > 1e-6, (label, m)
        n += 1
    assert n > 20


def test_two_maps_cases():
    raw, cor, tor, ref, n_types = GR.two_maps_case()
    assert n_types == 5 and all(om is not None for om in ref.fits)
    assert np.all(tor[np.isin(cor, (3, 17))] == -1) and np.sum(tor >= 0) < np.sum(cor >= 0)
    und = ref.undecided_rows()
    assert len(und) <= 0.005 * ref.fitted_rows(), (len(und), ref.fitted_rows())
    raw, cor, tor, ref, n_types = GR.two_maps_twin_case()
    assert n_types == 4 and len(ref.undecided_rows()) == 0   # every tie a twin tie: `choose` is compared as well


def test_the_end_to_end_fixture_is_decided_by_no_rounding():
    """No two-type partition of the fixture's barcodes leaves the oracle without undecided rows: the fixture holds deliberate ties,
    fragments with one score on loci 6 and 7, and every barcode has one.  They are EXACT ties on both sides, so every row of every
    barcode is compared: in each type the two loci hold the same sequence of (score, ambiguous) in ascending row order, so any order of
    additions that depends on the number of entries alone — the oracle's, and each class's of the device — gives both columns the same
    bits, and the two z of such a fragment are equal (0.5 to a rounding).  Every undecided row of the oracle is such a tie, none a near-tie."""
    ts, cor, tor, ref = GR.e2e_case()
    assert list(ts.barcodes).count(GR.E2E_OMITTED) == 1 and len(ts.barcodes) == 5
    omitted = list(ts.barcodes).index(GR.E2E_OMITTED)
    assert np.all(tor[cor == omitted] == -1) and np.all(tor[(cor >= 0) & (cor != omitted)] >= 0)
    assert all(om is not None for om in ref.fits) and sorted(om.n_iter for om in ref.fits)[-1] > GR.SP_LOOK
    raw = sp.csr_matrix(ts.raw_scores)
    z = ref.z()
    und = ref.undecided_rows()
    assert len(und) > 0
    for i in und:
        cols, v = z[i].indices, z[i].data
        assert len(v) == 2 and v[0] == v[1] and abs(v[0] - 0.5) < 1e-15, (i, v)
        sub = raw[np.flatnonzero(tor == tor[i])]
        amb = np.diff(sub.indptr) > 1
        seqs = []
        for j in cols:
            col = sub[:, j].tocoo()
            order = np.argsort(col.row)
            seqs.append((col.data[order].tolist(), amb[col.row[order]].tolist()))
        assert seqs[0] == seqs[1], (i, cols)
