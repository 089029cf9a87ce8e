"""bench.py's host-side pieces: the K-frame sequence built by host threads equals the frames built one by one, and --dump-outputs
writes float32 .npy files with a fixed, seeded sample of raw."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_frame_batches_threads_build_the_same_frames():
    import bench
    from invr import scene
    cpu, dev = bench.frame_batches(48, 1.8, 3, 'cpu')
    assert len(cpu) == len(dev) == 3
    for k in range(3):
        bnp, _ = scene.make_scene(48, 48, seed=0, frame=(3 + 7 * k) % 100, cam_dist=1.8, pose_seed=k)
        ref = scene.to_torch(bnp)
        assert sorted(ref) == sorted(cpu[k])
        for key in ref:
            assert torch.equal(ref[key], cpu[k][key]), (k, key)
            assert torch.equal(ref[key], dev[k][key]), (k, key)


def test_dump_outputs_writes_float32_maps_and_a_seeded_raw_sample(tmp_path):
    import bench
    n, S = 300, 1000                                       # 300,000 raw rows: more than RAW_SAMPLE_ROWS
    g = torch.Generator().manual_seed(0)
    full = torch.rand(n, 4, generator=g)
    local = {'rgb_map': full[:, :3].clone(), 'acc_map': full[:, 3].clone(), 'raw': torch.rand(n * S, 4, generator=g),
             'stats': torch.zeros(16, dtype=torch.int32)}
    bench.dump_outputs(str(tmp_path / 'a'), full, local)
    bench.dump_outputs(str(tmp_path / 'b'), full, local)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['acc_map.npy', 'raw_sample.npy', 'rgb_map.npy']
    a = {nm: np.load(tmp_path / 'a' / nm) for nm in names}
    assert all(v.dtype == np.float32 for v in a.values())
    assert np.array_equal(a['rgb_map.npy'], full[:, :3].numpy()) and np.array_equal(a['acc_map.npy'], full[:, 3].numpy())
    raw = a['raw_sample.npy']
    assert raw.shape == (bench.RAW_SAMPLE_ROWS, 4)
    # the sample is a fixed set of distinct rows of raw, in row order, the same in every run
    rows = {tuple(r) for r in local['raw'].numpy().tolist()}
    assert all(tuple(r) in rows for r in raw[::997].tolist())
    assert len({tuple(r) for r in raw.tolist()}) == raw.shape[0]
    assert np.array_equal(raw, np.load(tmp_path / 'b' / 'raw_sample.npy'))
    assert sum(os.path.getsize(tmp_path / 'a' / nm) for nm in names) < 64 << 20


def test_dump_outputs_without_raw(tmp_path):
    import bench
    full = torch.rand(10, 4)
    bench.dump_outputs(str(tmp_path), full, {'rgb_map': full[:, :3], 'acc_map': full[:, 3]})
    assert sorted(os.listdir(tmp_path)) == ['acc_map.npy', 'rgb_map.npy']
