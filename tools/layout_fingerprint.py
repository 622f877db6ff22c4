"""What tsem_build_layout made, and what runs on it, as text lines that two builds of the library can be compared by.

    TSEM_LIB=<library> python tools/layout_fingerprint.py --out DIR      one run (a fresh process per library): DIR/lines.txt, DIR/values.npz
    python tools/layout_fingerprint.py --compare OLD1 OLD2 NEW           two runs of the old library against one of the new

One line per item and case: the 46 fields of layout_info(extended=True), a SHA-256 over the decoded (row slot << 16 | column slot) words of every
sub-block (as stored where the fill is the row-order fill, every sub-block sorted where it is k_sb_fill, whose order within a strand
is the atomics'), the bits of pi, theta and lnl after 3 em_steps, and the column sums of reassign('exclude').  Every case asserts
from layout_info() that the branch it was built for was taken.

--compare: a line that the two old runs agree on must be the same in the new run.  A line they differ in (fp64 LDS atomics without
option "reproducible") is compared by value at the tolerance of tests/test_gpu_parity.py (RTOL 1e-9 relative; 1e-12 absolute for
the column sums); lnl and the column sums are computed from pi and theta, so they are in that class wherever the case's pi or theta
is, whether or not the two old runs happened to agree on them.  k_sb_fill deals the entries of a column that has several slots
(hot_cols > 0) over them in the atomics' order: the sorted words of such a layout differ between two runs of ONE library, so for
these cases the `subblock_rows` line (the row halves of the words, sorted) is what must be equal, and the `*_hot_split0` cases
repeat them without split columns, where the sorted words must be."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
RTOL = 1e-9


def const_len(n):
    """a length table (synthetic.poisson_cdf_u32) that gives every row n entries"""
    return np.zeros(n, np.uint32)


def cases():
    """(name, matrix, options, rebuild, check): matrix = (rows, K, length table, distribution, unique fraction) for Engine.generate, or
    'long_row'; rebuild = None | 'prepare_likelihood' | 'fallback_twopass'; check(info, mem) is what shows that the branch was taken"""
    from telescope_amd.synthetic import poisson_cdf_u32
    p40, p10 = poisson_cdf_u32(40), poisson_cdf_u32(10)
    small, big = (5000, 3000, p40, 1, 0.05), (70000, 3000, p40, 1, 0.05)
    out = [('big', big, (), None, lambda i, m: i['N_amb'] >= 65536 and i['fused'] == 1 and i['value_bytes'] == 2),
           ('small', small, (), None, lambda i, m: i['N_amb'] < 65536 and i['fused'] == 1 and i['value_bytes'] == 2 and i['row_order'] == 1)]
    for g, n in ((1, 10), (2, 24), (4, 48), (8, 100), (16, 200)):   # lanes per row of k_row_partcounts: the rule of k_colsig's, which layout_info has
        out.append(('lanes%d' % g, (5000, 3000, const_len(n), 0, 0.05), (), None, lambda i, m, g=g: i['colsig_lanes'] == g and i['fused'] == 1))
    zipf = (5000, 3000, p10, 1, 0.05)
    out += [('hot', zipf, (), None, lambda i, m: i['hot_cols'] > 0 and i['fused'] == 1),
            ('hot_split0', zipf, (('hot_split', 0),), None, lambda i, m: i['hot_cols'] == 0 and i['fused'] == 1),
            ('no_ambiguous', (5000, 3000, p40, 1, 1.0), (), None, lambda i, m: i['nb'] == 0 and i['N_amb'] == 0),
            ('wide', (3000, 491521 + 64, p40, 0, 0.05), (), None, lambda i, m: i['row_pass_em'] == 1 and i['nb'] == 0),
            ('fp64', small, (('value_format', 1),), None, lambda i, m: i['index_bytes'] == 3 and i['value_bytes'] == 8 and i['fused'] == 1)]
    out.append(('fp64_quad', small, (('value_format', 1), ('index_format', 2)), None,        # the quad index, which auto takes at 1 GiB only
                lambda i, m: i['index_format'] == 2 and i['index_bytes'] == 2 and i['value_bytes'] == 8 and i['fused'] == 1))
    for p in (2, 4, 5, 8):
        out.append(('parts%d' % p, small, (('parts', p),), None, lambda i, m, p=p: i['P'] == p and i['fused'] == 1))
    for p, g in ((2, 2), (2, 3), (4, 2), (4, 3)):
        out.append(('parts%d_geo%d' % (p, g), small, (('parts', p), ('geometry', g)), None, lambda i, m, p=p, g=g: i['P'] == p and i['geometry'] == g and i['fused'] == 1))
    out += [('split', small, (('parts', 5), ('split', 1)), None, lambda i, m: i['split'] == 1 and i['P'] == 5 and i['fused'] == 1),
            ('reproducible1', small, (('reproducible', 1),), None, lambda i, m: i['reproducible'] >= 1 and i['exact_single'] == 1 and i['fused'] == 1),
            ('reproducible2', small, (('reproducible', 2),), None, lambda i, m: i['reproducible'] >= 1 and i['exact_single'] == 0 and i['fused'] == 1),
            ('use_likelihood', small, (('use_likelihood', 1),), None, lambda i, m: i['lnl_fused'] == 1 and i['fused'] == 1),
            ('twopass', small, (('em_kernel', 1),), None, lambda i, m: i['fused'] == 0 and i['index_bytes'] == 4 and i['value_bytes'] == 8),
            ('sorted_fill0', small, (('sorted_fill', 0),), None, lambda i, m: i['row_order'] == 0 and i['fused'] == 1),
            ('deconflict0', small, (('deconflict', 0),), None, lambda i, m: i['row_order'] == 1 and i['fused'] == 1),
            ('report_kernel0', small, (('report_kernel', 0),), None, lambda i, m: m['ids'] == 0 and i['fused'] == 1),
            ('drop_csr_indices', small, (('drop_csr_indices', 1),), None, lambda i, m: m['csr_indices'] == 0 and m['ids'] > 0 and i['fused'] == 1),
            ('twopass_hot_split0', small, (('em_kernel', 1), ('hot_split', 0)), None, lambda i, m: i['fused'] == 0 and i['hot_cols'] == 0),
            ('sorted_fill0_hot_split0', small, (('sorted_fill', 0), ('hot_split', 0)), None, lambda i, m: i['row_order'] == 0 and i['fused'] == 1 and i['hot_cols'] == 0),
            ('block_rows64', small, (('block_rows', 64),), None, lambda i, m: i['R'] == 64 and i['fused'] == 1),
            ('long_row', 'long_row', (), None, lambda i, m: i['fused'] == 0 and i['N_amb'] > 0),   # a row past the register tile: fixed blocks
            ('prepare_likelihood', small, (), 'prepare_likelihood', lambda i, m: i['lnl_fused'] == 1 and i['fused'] == 1),
            ('fallback_twopass', small, (), 'fallback_twopass', lambda i, m: i['fused'] == 0 and i['fallbacks'] == 1),
            ('fallback_twopass_hot_split0', small, (('hot_split', 0),), 'fallback_twopass', lambda i, m: i['fused'] == 0 and i['fallbacks'] == 1 and i['hot_cols'] == 0)]
    return out


def long_row_matrix():
    """2000 generated rows of ~20 entries in 5000 columns and one hand-made row of 3600: more than a register tile takes (3584)"""
    from telescope_amd import synthetic
    ip, ix, rw = synthetic.generate(2000, 5000, 20, seed=7, dist='uniform', uniq_frac=0.05)
    cols = np.arange(0, 3600, dtype=np.int32)
    return (np.append(ip, ip[-1] + len(cols)), np.concatenate([ix, cols]),
            np.concatenate([rw, (139 + cols % 162).astype(np.uint16)]), 5000)


def subblock_digest(eng, info):
    h, hr = hashlib.sha256(), hashlib.sha256()
    cap = max(8192, int(info['max_subblock']) + 64, int(info['nnz_pad']) // max(1, int(info['nb'] * info['P'])) * 64)
    n = 0
    for b in range(int(info['nb'])):
        for p in range(int(info['P'])):
            w = eng.debug_subblock(b, p, cap=cap)
            assert len(w) < cap, 'sub-block (%d, %d) fills the buffer of %d words' % (b, p, cap)
            h.update(np.int64(len(w)).tobytes())
            h.update((w if info['row_order'] else np.sort(w)).tobytes())
            hr.update(np.sort(w >> 16).tobytes())
            n += len(w)
    return h.hexdigest(), hr.hexdigest(), n


def run(out_dir):
    from telescope_amd._lib import Engine, Z_CUR
    from telescope_amd.likelihood import score_lut
    os.makedirs(out_dir, exist_ok=True)
    lines, values = [], {}
    todo = cases()
    for name, mat, options, rebuild, check in todo:
        eng = Engine(0)
        for key, v in options:
            eng.set_option(key, v)
        if mat == 'long_row':
            ip, ix, rw, k = long_row_matrix()
            eng.load_scores(ip, ix, rw, k, None)
        else:
            rows, k, cdf, dist, uniq = mat
            eng.generate(0, rows, k, cdf, 42, dist, uniq)
        eng.set_lut(score_lut(eng.max_score()))
        stats, pisum0, cnt, hsh = eng.rowstats()
        eng.set_model(stats, pisum0, cnt, hsh, 0.0, 200000.0)
        if rebuild:
            getattr(eng, rebuild)()
        info, mem = eng.layout_info(extended=True), eng.device_memory()['resident']
        assert check(info, mem), ('case %s did not take its branch' % name, info, mem)
        lines += ['%s info.%s %d' % (name, key, v) for key, v in info.items()]
        lines += ['%s resident.%s %d' % (name, key, v) for key, v in mem.items()]
        words, row_halves, n = subblock_digest(eng, info)
        lines.append('%s subblocks %s (%d words, %s)' % (name, words, n, 'as stored' if info['row_order'] else 'sorted'))
        lines.append('%s subblock_rows %s' % (name, row_halves))
        eng.em_steps(3, False)
        pi, theta = eng.get_params(Z_CUR)
        lnl = np.array([eng.final_lnl()])
        excl = eng.reassign('exclude', 0.9, Z_CUR)[0]
        for key, a in (('pi', pi), ('theta', theta), ('lnl', lnl), ('exclude', excl)):
            values['%s %s' % (name, key)] = a
            lines.append('%s %s %s' % (name, key, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()))
        lines.append('%s fallbacks_after_em %d' % (name, eng.layout_info()['fallbacks']))
        eng.close()
        print('%-20s P %d Kp %d R %d nb %d fused %d geometry %d value_bytes %d index_bytes %d row_order %d hot_cols %d lnl %r' % (
            name, info['P'], info['Kp'], info['R'], info['nb'], info['fused'], info['geometry'], info['value_bytes'], info['index_bytes'],
            info['row_order'], info['hot_cols'], float(lnl[0])), flush=True)
    with open(os.path.join(out_dir, 'lines.txt'), 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    np.savez(os.path.join(out_dir, 'values.npz'), **values)
    print('%d lines, %d cases -> %s' % (len(lines), len(todo), out_dir))


def compare(old1, old2, new):
    def load(d):
        rows = [ln.rstrip('\n') for ln in open(os.path.join(d, 'lines.txt'))]
        return {' '.join(r.split(' ')[:2]): r for r in rows}, np.load(os.path.join(d, 'values.npz'))
    (a, va), (b, vb), (c, vc) = load(old1), load(old2), load(new)
    assert list(a) == list(b) == list(c), 'the runs do not list the same items'
    equal = toler = 0
    worst, bad, dealt = 0.0, [], []
    loose = set(key.split(' ')[0] for key in a if key.split(' ')[1] in ('pi', 'theta') and a[key] != b[key])   # cases whose parameters are in the tolerance class
    for key in a:
        name, item = key.split(' ')
        if item == 'subblocks' and a[key] != b[key] and a[name + ' info.row_order'].endswith(' 0') and not a[name + ' info.hot_cols'].endswith(' 0'):
            dealt.append(name)                               # (k_sb_fill with split columns: see the module's text)
            continue
        if a[key] == b[key] and not (name in loose and item in ('lnl', 'exclude')):
            equal += 1
            if c[key] != a[key]:
                bad.append('%s\n    old %s\n    new %s' % (key, a[key], c[key]))
            continue
        toler += 1
        if key not in va.files:
            bad.append('%s differs between the two old runs and is no array: %s | %s' % (key, a[key], b[key]))
            continue
        x, y, z = va[key], vb[key], vc[key]
        atol = 1e-12 if key.endswith(' exclude') else 0.0
        err = lambda p, q: float(np.max(np.abs(p - q) / np.maximum(np.abs(q), 1e-300))) if p.size else 0.0   # noqa: E731
        worst = max(worst, err(z, x))
        print('tolerance class: %-28s old/old %.3g  new/old %.3g relative' % (key, err(y, x), err(z, x)))
        if not np.allclose(z, x, rtol=RTOL, atol=atol):
            bad.append('%s: new against old beyond rtol %g' % (key, RTOL))
    print('%d lines: %d must be equal, %d in the tolerance class (largest new/old difference %.3g relative), %d sub-block digests of k_sb_fill with '
          'split columns that the old library does not reproduce (%s); %d failures' % (len(a), equal, toler, worst, len(dealt), ', '.join(dealt), len(bad)))
    for t in bad:
        print('DIFFERENT ' + t)
    return 1 if bad else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out')
    ap.add_argument('--compare', nargs=3, metavar=('OLD1', 'OLD2', 'NEW'))
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out) or 0)
