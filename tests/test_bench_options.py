"""bench.py's run modes: a plain run times the steps and prints the headline, `--full` adds the legs that cost work of their own, and
`--dump-outputs DIR` writes what the timed call computed so that two builds can be compared output for output."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _parse(monkeypatch, *argv):
    sys.path.insert(0, ROOT)
    bench = importlib.import_module('bench')
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
    return bench.parse()


def test_plain_is_the_default_and_steps_must_be_positive(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'out')
    assert a.full is True and a.dump_outputs == 'out'
    for bad in (('--steps', '0'), ('--warmup', '-1')):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *bad)


def _plain(tmp_path, tag):
    out = str(tmp_path / tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--rows', '1000000', '--steps', '5', '--warmup', '2',
                        '--dump-outputs', out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line, {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


@pytest.mark.gpu
def test_plain_line_and_dumped_outputs(gpu_device, tmp_path):
    """A plain run: `steps` timed EM iterations after `warmup` ones, the headline keys, none of the --full legs; the dump holds the
    parameters the timed call left (the same numbers as the line's `check` fold) and a z sample, float64, and a second run agrees."""
    one, a = _plain(tmp_path, 'a')
    two, b = _plain(tmp_path, 'b')
    for line in (one, two):
        assert line['steps'] == 5 and line['warmup'] == 2 and line['check']['iterations'] == 7
        assert line['unit'] == 'iter/s' and line['higher_is_better'] is True and line['dtype'] == 'f64'
        assert abs(line['value'] * line['ms_per_step'] - 1e3) < 1e-6 * 1e3
        assert line['full'] is False and line['phase_us'] is None and line['whole_em_call'] is None and line['report_pass'] is None
        assert not any(k in line for k in ('cpu_baseline', 'code16_layout', 'precision_sweep', 'reproducible_mode'))
        assert line['outputs_dumped'] == sorted(a)
    assert sorted(a) == ['pi', 'pi_init', 'theta', 'theta_init', 'z_sample', 'z_sample_indptr', 'z_sample_rows']
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    # the inputs are the same in both runs; the column sums of the default mode are atomics, so the outputs agree to rounding
    # (bench.py's CHECK_RTOL), not bit for bit
    for k in a:
        assert a[k].dtype == np.float64 and a[k].shape == b[k].shape, k
        if k in ('z_sample_rows', 'z_sample_indptr'):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert np.allclose(a[k], b[k], rtol=1e-11, atol=0), (k, np.max(np.abs(a[k] - b[k])))
    k_cols = 30_000
    assert a['pi'].shape == a['theta'].shape == (k_cols,)
    assert a['pi'].sum() == one['check']['pi_sum']
    pw = np.dot(a['pi'], np.arange(1, k_cols + 1, dtype=np.float64) / k_cols)
    assert abs(pw - one['check']['pi_weighted']) <= 1e-14 * abs(pw)
    rows, off, z = a['z_sample_rows'], a['z_sample_indptr'].astype(np.int64), a['z_sample']
    assert len(rows) == 16384 and np.all(np.diff(rows) > 0) and off[0] == 0 and off[-1] == len(z) > len(rows)
    kept = z >= 0
    assert np.all(kept | (z == -1)) and np.all(z[kept] <= 1.0)
    sums = np.add.reduceat(np.where(kept, z, 0.0), off[:-1])
    full_rows = np.logical_and.reduceat(kept, off[:-1])
    assert np.allclose(sums[full_rows], 1.0, rtol=0, atol=1e-12)     # a row's posteriors add up to one
