"""`--updated_sam`, `-m gpu`: the device tag pass (tsem_entry_tags, RP_TAGS of k_rowpass) and its PHRED lookup against numpy and
`tl.lookup`, and `assign --updated_sam` / `sc assign --updated_sam` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLD, ROOT, Opts, case_matrix, case_names, load_case

pytestmark = pytest.mark.gpu
METHODS = ('exclude', 'choose', 'average', 'conf', 'unique', 'all')


def test_updated_sam_debug_phred_matches_numpy(gpu_device):
    from telescope_amd import _lib, bam_out
    tab = bam_out.phred_table()
    one = int(np.float64(1.0).view(np.uint64))
    bits = tab.view(np.uint64).astype(np.int64)
    near = np.concatenate([bits + d for d in range(-2, 3)])
    near = near[(near >= 0) & (near < one)].astype(np.uint64).view(np.float64)
    rng = np.random.default_rng(3)
    p = np.concatenate([near, rng.random(200_000), [0.0, 0.9, 0.999999, 1.0, 1.0000000000000002, 0.125, 0.2]])
    got = _lib.debug_phred(p, tab, device=gpu_device)
    want = np.array([bam_out.phred_scalar(x) for x in p])
    assert np.array_equal(got, want), p[np.flatnonzero(got != want)[:5]]


def _tiles(n, rng):
    """arbitrary cuts of [0, n): empty tiles, one-row tiles, the rest random"""
    cuts = sorted(set([0, n] + list(rng.integers(0, n + 1, size=min(n, 6))) + ([1, 2] if n > 2 else [])))
    out = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += [(a, a), (a, b)]
    return out


def _restated(tl, method, assignment):
    """tag words of every stored entry from tl.lookup (z, reassign value) and the host PHRED table"""
    from telescope_amd import bam_out
    r = tl._need_raw()
    ridx = np.repeat(np.arange(tl.N), np.diff(r.indptr))
    prob, val = tl.lookup(ridx, r.indices, method, 0.9, assignment=assignment)
    return bam_out.tag_word(prob, val)


LAYOUTS = [{}, {'value_format': 1}, {'hot_split': 0}, {'drop_csr_indices': 1}]


@pytest.mark.parametrize('layout', range(len(LAYOUTS)))
@pytest.mark.parametrize('name', case_names(full_only=True))
def test_updated_sam_entry_tags_equal_lookup(gpu_device, name, layout):
    """the tag pass restated from `tl.lookup` — the same kernel in another mode, so this ties the two entry points together and
    nothing more; the outside reference of the words (exact z, the oracle's assignment, the host quantiser, on all entries) lives
    in tests/test_gpu_rowpass_entries.py"""
    from telescope_amd.likelihood import TelescopeLikelihood
    c = load_case(name)
    raw = case_matrix(c)
    tl = TelescopeLikelihood(raw, Opts(c), device=gpu_device, engine_options=LAYOUTS[layout] or None)
    tl.em()
    rng = np.random.default_rng(layout)
    for method in METHODS:
        a = tl.reassign(method, 0.9)
        want = _restated(tl, method, a)
        got = [tl.entry_tags(r0, r1, method, 0.9, assignment=a) for r0, r1 in _tiles(tl.N, rng)]
        got = np.concatenate(got) if got else np.zeros(0, np.uint32)
        assert np.array_equal(got, want), (name, method, np.flatnonzero(got != want)[:5])
        tiles = list(tl.entry_tag_tiles(method, 0.9, assignment=a, tile_bytes=4 * 37))
        assert tiles[0][0] == 0 and tiles[-1][1] == tl.N and all(t[1] == u[0] for t, u in zip(tiles, tiles[1:]))
        assert np.array_equal(np.concatenate([t[2] for t in tiles]), want), (name, method, 'tiles')


@pytest.mark.parametrize('seed,kw', [(1, {}), (3, dict(long_rows=40, n=3000)), (5, dict(max_len=250, n=1500, k=600))])
def test_updated_sam_entry_tags_on_near_ties(gpu_device, seed, kw):
    """near-tie rows (test_gpu_round6): the tag pass decides them in its FIX launch like the reassign pass of tsem_rows_lookup"""
    from test_gpu_round6 import _near_tie_matrix
    from telescope_amd import _lib, bam_out
    from telescope_amd.likelihood import TelescopeLikelihood, score_lut
    raw, pi, theta = _near_tie_matrix(seed, **kw)
    n, k = raw.shape
    eng = _lib.Engine(gpu_device)
    eng.load_scores(raw.indptr, raw.indices, raw.data.astype(np.uint16), k, score_lut(int(raw.data.max())))
    tl = TelescopeLikelihood.from_engine(eng, Opts(max_iter=1, em_epsilon=0.0))      # (the model the parameters go into)
    tl._raw = raw
    eng.set_params(pi, theta)
    tab = bam_out.phred_table()
    rows = np.arange(n, dtype=np.int32)
    rng = np.random.default_rng(seed)
    picks = rng.integers(0, 3, n).astype(np.int32)
    for method in METHODS:
        pk = picks if method == 'choose' else None
        z, m = eng.rows_lookup(method, 0.9, _lib.Z_CUR, rows, raw.indptr, pk)
        want = bam_out.tag_word(np.where(z < 0, 0.0, z), m)
        got = []
        for r0, r1 in _tiles(n, rng):
            got.append(eng.entry_tags(method, 0.9, _lib.Z_CUR, r0, r1, tab, None if pk is None else pk[r0:r1],
                                      n_out=raw.indptr[r1] - raw.indptr[r0]))
        assert np.array_equal(np.concatenate(got), want), (method, np.flatnonzero(np.concatenate(got) != want)[:5])
    eng.close()


class _O(object):
    def __init__(self, samfile, gtffile, outdir, mode, **kw):
        self.samfile, self.gtffile, self.outdir, self.exp_tag = samfile, gtffile, outdir, 'telescope'
        self.attribute, self.no_feature_key, self.overlap_mode, self.overlap_threshold = 'locus', '__no_feature', 'threshold', 0.2
        self.stranded_mode, self.reassign_mode, self.conf_prob, self.updated_sam = 'None', mode, 0.9, True
        self.em_epsilon, self.max_iter, self.pi_prior, self.theta_prior, self.use_likelihood = 1e-7, 100, 0, 200000, False
        self.reproducible, self.device, self.version = False, 0, 'test'
        self.__dict__.update(kw)

    def outfile_path(self, suffix):
        return os.path.join(self.outdir, '%s-%s' % (self.exp_tag, suffix))


def _records(path):
    from telescope_amd import loader
    _, recs, header = loader.read_bam(path, raw=True)
    return [s.raw for s in recs], header


CASES = [('loader_mixed.bam', 'loader_mixed.gtf', False), ('sc_mixed.bam', 'sc_mixed.gtf', True),
         ('bundled_alignment.bam', 'bundled_annotation.gtf', False)]


@pytest.mark.parametrize('mode', ['exclude', 'choose', 'average', 'conf', 'unique'])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_updated_sam_matches_a_restatement_from_lookup(gpu_device, tmp_path, case, mode):
    """update_sam's records = model.py:495-518 applied to the tmp BAM with `tl.lookup`'s z and assignment (the same fresh
    `reassign` draw for choose), record for record; the header is the input's plus one @PG line."""
    from telescope_amd import bam_out, cli, loader
    from telescope_amd.run_container import Telescope, scTelescope
    bam, gtf, sc = CASES[case]
    o = _O(os.path.join(GOLD, bam), os.path.join(GOLD, gtf), str(tmp_path), mode, barcode_tag='CB')
    ts = scTelescope(o) if sc else Telescope(o)
    ts.load_alignment(loader.Annotation(o.gtffile, o.attribute, o.stranded_mode))
    np.random.seed(ts.get_random_seed())
    tl, _ = cli.build_model(ts.raw_scores, o)
    tl.em()
    ts.output_report(tl, o.outfile_path('run_stats.tsv'), o.outfile_path('TE_counts.tsv'))
    state = np.random.get_state()
    ts.update_sam(tl, o.outfile_path('updated.bam'), command_line='telescope assign test')
    np.random.set_state(state)
    a = tl.reassign(mode, 0.9)
    tmp, header = _records(ts.tmp_bam)
    got, h2 = _records(o.outfile_path('updated.bam'))
    assert h2['text'] == bam_out.header_with_pg(header['text'], 'test', 'telescope assign test')
    assert h2['refs_block'] == header['refs_block']
    _, segs, _ = loader.read_bam(ts.tmp_bam, raw=True)
    want = []
    for _code, pairs in loader._fragments(segs):
        ridx = ts.read_index[pairs[0].r1.qname]
        for p in pairs:
            recs = p.records()
            if p.is_unmapped:
                want += recs
                continue
            zt = bam_out.get_tag(recs[0], 'ZT')
            w = 0
            if zt == 'PRI':
                prob, val = tl.lookup([ridx], [ts.feat_index[bam_out.get_tag(recs[0], 'ZF')]], mode, 0.9, assignment=a)
                w = int(bam_out.tag_word(prob, val)[0])
            want += bam_out.update_pair(recs, zt, w)
    assert len(got) == len(want) == len(tmp)
    for g, w in zip(got, want):
        assert bam_out.record_text(g) == bam_out.record_text(w)
        assert g == w


def test_updated_sam_bundled_cli_run_keeps_the_reports(gpu_device, tmp_path):
    """the bundled run with --updated_sam: the same log-likelihood line and the same TSVs as without it, and the updated BAM holds
    every record of the tmp BAM"""
    from telescope_amd import bam_out
    args = [os.path.join(GOLD, 'bundled_alignment.bam'), os.path.join(GOLD, 'bundled_annotation.gtf')]
    outs = {}
    for flag in ([], ['--updated_sam']):
        d = str(tmp_path / ('u' if flag else 'p'))
        r = subprocess.run([sys.executable, '-m', 'telescope_amd', 'assign'] + args + flag + ['--outdir', d], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        assert 'Final log-likelihood: 95252.596293.' in r.stderr
        outs[bool(flag)] = d
    for f in ('telescope-run_stats.tsv', 'telescope-TE_counts.tsv'):
        assert open(os.path.join(outs[True], f)).read() == open(os.path.join(outs[False], f)).read()
    assert not os.path.exists(os.path.join(outs[False], 'telescope-updated.bam'))
    upd, h = _records(os.path.join(outs[True], 'telescope-updated.bam'))
    tmp, h0 = _records(os.path.join(outs[True], 'telescope-tmp_tele.bam'))
    other, _ = _records(os.path.join(outs[True], 'telescope-other.bam'))
    inp, hin = _records(args[0])
    assert len(upd) == len(tmp) and len(tmp) + len(other) <= len(inp)
    assert h['text'].startswith(hin['text']) and h['text'].count('\n@PG') == hin['text'].count('\n@PG') + 1
    assert [bam_out.qname_of(r) for r in upd] == [bam_out.qname_of(r) for r in tmp]
    assert all(bam_out.get_tag(r, 'YC') is not None for r in upd if not bam_out.flag_of(r) & 4)


def _ulps_apart(m1, m2):
    """how many float64 steps separate the P ranges whose PHRED scores are m1 and m2 (0: adjacent or equal)"""
    from telescope_amd import bam_out
    tab = bam_out.phred_table()
    one = int(np.float64(1.0).view(np.uint64))

    def rng(m):                                        # [first, last] bit patterns of the P with phred(P) == m
        if m == 255:
            return one, one
        lo = 0 if m == 0 else int(tab[m - 1].view(np.uint64))
        hi = (int(tab[m].view(np.uint64)) if m < len(tab) else one) - 1
        return lo, hi
    (a0, a1), (b0, b1) = sorted([rng(m1), rng(m2)])
    return max(0, b0 - a1 - 1)


def _mapq_as_reference(g, w):
    """`g` with the reference's MAPQ where that is the only difference and the two scores are the PHRED of z values at most 4 ulp
    apart: the engine's pi / theta may differ from scipy's in their last bit, which moves z by an ulp or so — and next to
    z = 1 one ulp is the difference between MAPQ 255 and 160.  Every other field must match exactly."""
    gf, wf = g.split('\t'), w.split('\t')
    if g == w or len(gf) != len(wf) or gf[:2] + gf[3:] != wf[:2] + wf[3:]:
        return g
    return w if _ulps_apart(int(gf[2]), int(wf[2])) <= 4 else g


@pytest.mark.parametrize('mode', ['exclude', 'choose', 'average', 'conf', 'unique'])
@pytest.mark.parametrize('name', ['loader_mixed', 'sc_mixed', 'updated_mixed', 'bundled'])
def test_updated_sam_cli_matches_the_reference(gpu_device, tmp_path, name, mode):
    """`assign --updated_sam` (`sc assign` for sc_mixed) on the GPU: -other.bam, -tmp_tele.bam and -updated.bam hold the records the
    reference's own _load_sequential / update_sam write (tools/make_updated_sam_fixture.py), the header is the input's plus one @PG"""
    from telescope_amd import cli
    from test_updated_sam_golden import CASES, expected, inputs, same, texts
    exp = expected()[name]
    bam, gtf = inputs(name)
    out = str(tmp_path)
    argv = (['sc'] if CASES[name] else []) + ['assign', bam, gtf, '--updated_sam', '--reassign_mode', mode, '--outdir', out, '--quiet']
    assert cli.main(argv) == 0
    _, hin = texts(bam)
    for key in ('other', 'tmp_tele', 'updated'):
        got, h = texts(os.path.join(out, 'telescope-%s.bam' % key))
        want = exp[key if key != 'updated' else 'updated_' + mode]
        if key == 'updated' and isinstance(want, list) and len(got) == len(want):
            got = [_mapq_as_reference(g, w) for g, w in zip(got, want)]
        diff = [(g, w) for g, w in zip(got, want) if g != w] if isinstance(want, list) else []
        assert same(got, want), (name, mode, key, diff[:3])
        if key == 'updated':
            assert h['text'].startswith(hin['text']) and h['text'].count('@PG\t') == hin['text'].count('@PG\t') + 1
            assert h['text'].splitlines()[-1].startswith('@PG\tID:telescope' + ('.1' if name == 'updated_mixed' else '') + '\tPN:telescope\t')
        else:
            assert h == hin
