"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only; the dump holds what the last timed
step returned, float32, within the size limit (a fixed seeded row sample beyond it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location('occ4d_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_and_samples_beyond_the_limit(tmp_path, monkeypatch):
    bench = _bench()
    out = torch.arange(40 * 5, dtype=torch.float32).reshape(40, 5)
    bench.dump_outputs(str(tmp_path / 'all'), {'implicit_output': out}, 0, 1)
    got = np.load(tmp_path / 'all' / 'implicit_output.npy')
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy())
    assert sorted(os.listdir(tmp_path / 'all')) == ['implicit_output.npy']

    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 40 * 5 * 4 // 2)           # half of it fits: a 20-row sample
    for rep in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / rep), {'implicit_output': out}, 0, 1)
    rows = np.load(tmp_path / 'a' / 'implicit_output_rows.npy')
    got = np.load(tmp_path / 'a' / 'implicit_output.npy')
    assert rows.dtype == np.float64 and rows.shape == (20,) and np.all(np.diff(rows) > 0)
    assert np.array_equal(got, out.numpy()[rows.astype(np.int64)])
    assert np.array_equal(rows, np.load(tmp_path / 'b' / 'implicit_output_rows.npy'))     # the same sample every run

    bench.dump_outputs(str(tmp_path / 'ranks'), {'implicit_output': out}, 1, 2)         # N > 1: one file set per rank
    assert sorted(os.listdir(tmp_path / 'ranks')) == ['implicit_output_rank1.npy', 'implicit_output_rows_rank1.npy']


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    proc = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1',
                           '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, proc.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['steps'] == 2 and d['n_gpus'] == 1 and d['unit'] == 'query-points/s' and d['higher_is_better'] is True
    assert d['dtype'] == 'f32' and d['ms_per_step'] > 0
    assert abs(d['value'] - 534528 / (d['ms_per_step'] * 1e-3)) / d['value'] < 1e-6
    for leg in ('roofline', 'pipeline', 'cpu_baseline', 'config4_single_gpu', 'alt_precision', 'carla_config3'):
        assert leg not in d, leg
    assert os.listdir(tmp_path) == ['implicit_output.npy']
    got = np.load(tmp_path / 'implicit_output.npy')
    assert got.dtype == np.float32 and got.shape == (534528, d['config']['outputs_per_query'])
    assert np.isfinite(got).all()
