"""GPU: a plain bench.py run (small model, small frame) times exactly --steps steps, prints the headline line without the --full
objects, and --dump-outputs gives the same arrays in two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '4', '--warmup', '1', '--res', '64',
           '--samples', '32', '--table-log2', '12', '--dump-outputs', str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_bench_run_and_dumped_outputs(tmp_path):
    line = _run(tmp_path / 'a')
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['metric'] == 'ray-samples/sec' and line['unit'] == 'ray-samples/s' and line['higher_is_better'] is True
    assert line['steps'] == 4 and line['repeats'] == 1 and line['ms_per_step'] > 0
    assert abs(line['timed_region_s'] * 1e3 / 4 - line['ms_per_step']) < 1e-9
    for k in ('roofline', 'path_roofline', 'stage_ms_per_step', 'replay_bit_exact', 'train_step', 'samples_64'):
        assert k not in line, k
    assert line['cpu_baseline'] is None
    n = line['config']['rays_per_frame'][-1]
    a = {nm: np.load(tmp_path / 'a' / (nm + '.npy')) for nm in ('rgb_map', 'acc_map', 'raw_sample')}
    assert a['rgb_map'].shape == (n, 3) and a['acc_map'].shape == (n,) and a['raw_sample'].shape[1] == 4
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert float(a['acc_map'].max()) > 0
    _run(tmp_path / 'b')
    for nm, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / 'b' / (nm + '.npy'))), nm
