"""Timing of the mesh path on the bench scene's full-size model (profiles/mesh_extraction.md): the occupancy volume on a voxel grid over
the frame's world bounds, then invr_mesh_count and invr_mesh_emit, each timed with events on the stream (median of --runs after
--warmup); the bytes every kernel has to move, from the shapes.  --once: one untimed pass (for a rocprofv3 --kernel-trace run).
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import invr  # noqa: E402,F401
from invr import _abi, mesh, scene  # noqa: E402
from invr.config import make_cfg  # noqa: E402
import bench  # noqa: E402


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    out = fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--voxel', type=float, default=0.005)
    ap.add_argument('--level', type=float, default=0.1)
    ap.add_argument('--runs', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--table-log2', type=int, default=None, help='debug: cap log2_hashmap_size')
    ap.add_argument('--once', action='store_true')
    args = ap.parse_args()
    dev = 'cuda:0'
    cfg = make_cfg(N_samples=128, **({'table_log2': args.table_log2} if args.table_log2 else {}))
    net = bench.build_model(cfg, dev)
    bnp, _ = scene.make_scene(512, 512, seed=0, frame=3, cam_dist=1.8, pose_seed=0)          # frame 0 of the bench sequence
    batch = {k: v.to(dev) for k, v in scene.to_torch(bnp).items()}
    L = _abi.lib()
    st = torch.cuda.current_stream()

    def one():
        t_fill, (vol, origin, voxel) = timed(lambda: mesh.occupancy_volume(net, batch, voxel_size=args.voxel), st)
        dims = (C.c_int32 * 3)(*vol.shape)
        nbytes = L.invr_mesh_workspace_bytes(dims)
        ws = mesh._aligned_bytes(nbytes, dev)
        counts = torch.empty(4, dtype=torch.int64, device=dev)
        o3, v3 = (C.c_float * 3)(*[float(x) for x in origin]), (C.c_float * 3)(*[float(x) for x in voxel])
        t_count, _ = timed(lambda: _abi.check(L.invr_mesh_count(_abi.ptr(vol), dims, args.level, _abi.ptr(ws, torch.uint8), nbytes,
                                                                _abi.ptr(counts, torch.int64), _abi.stream_ptr())), st)
        nv, nt = counts[:2].tolist()
        verts, tris = torch.empty(nv, 3, device=dev), torch.empty(nt, 3, dtype=torch.int32, device=dev)
        t_emit, _ = timed(lambda: _abi.check(L.invr_mesh_emit(_abi.ptr(vol), dims, o3, v3, args.level, _abi.ptr(ws, torch.uint8), nbytes,
                                                              _abi.ptr(verts), nv, _abi.ptr(tris, torch.int32), nt, _abi.ptr(counts, torch.int64),
                                                              _abi.stream_ptr())), st)
        assert counts.tolist() == [nv, nt, 0, 0]
        return dict(fill=t_fill, count=t_count, emit=t_emit), vol, nv, nt

    if args.once:
        one()
        torch.cuda.synchronize()
        return
    for _ in range(args.warmup):
        one()
    runs = [one() for _ in range(args.runs)]
    t, vol, nv, nt = runs[-1]
    n = vol.numel()
    npad = (vol.shape[0] + 2) * (vol.shape[1] + 2) * (vol.shape[2] + 2)
    med = {k: statistics.median(r[0][k] for r in runs) for k in t}
    out = {'voxel': args.voxel, 'level': args.level, 'dims': list(vol.shape), 'points': n, 'padded_points': npad,
           'nonzero_share': float((vol != 0).float().mean()), 'inside_share': float((vol >= args.level).float().mean()),
           'vertices': nv, 'triangles': nt, 'runs': args.runs, 'ms_median': med,
           'ms_all': {k: [round(r[0][k], 4) for r in runs] for k in t},
           # what each kernel has to move at least, from the shapes (B): the look-ups of emit's triangles are not counted
           'bytes': {'k_grid_points': 12 * n, 'k_mesh_classify': 4 * n + 2 * npad, 'k_mesh_reduce': 2 * npad, 'k_mesh_apply': 10 * npad,
                     'k_mesh_emit': 2 * npad + 12 * nv + 12 * nt}}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
