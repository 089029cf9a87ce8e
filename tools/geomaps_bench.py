"""Cost of the geometry maps on the bench frame (512 x 512 x 128, profiles/geometry_maps.md): Network.render_rays without and with
want_depth (the depth pass behind the compositing), with and without raw, and geomaps.geometry_maps with and without normals — all in
one process, the variants interleaved round by round, each call timed with events on the stream; medians and the spread over --runs
rounds after --warmup.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import invr  # noqa: E402,F401
from invr import geomaps, scene  # noqa: E402
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
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--samples', type=int, default=128)
    ap.add_argument('--level', type=float, default=0.5)
    ap.add_argument('--h', type=float, default=0.005)
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--table-log2', type=int, default=None, help='debug: cap log2_hashmap_size')
    args = ap.parse_args()
    dev = 'cuda:0'
    S = args.samples
    cfg = make_cfg(N_samples=S, **({'table_log2': args.table_log2} if args.table_log2 else {}))
    net = bench.build_model(cfg, dev)
    bnp, _ = scene.make_scene(args.res, args.res, seed=0, frame=3, cam_dist=1.8, pose_seed=0)          # frame 0 of the bench sequence
    batch = {k: v.to(dev) for k, v in scene.to_torch(bnp).items()}
    st = torch.cuda.current_stream()
    ro, rd, near, far = [batch[k][0].contiguous() for k in ('ray_o', 'ray_d', 'near', 'far')]
    with torch.no_grad():
        ctx = net.prepare(batch)
        full = net.render_rays(ctx, ro, rd, near, far, S, want_raw=False)
        cap = int(1.5 * int(full['stats'][0])) + 65536          # the survivor bound Renderer settles at
        render = lambda **kw: net.render_rays(ctx, ro, rd, near, far, S, max_active=cap, **kw)
        variants = {
            'render_raw': lambda: render(want_raw=True),
            'render_raw_depth': lambda: render(want_raw=True, want_depth=True, level=args.level),
            'render_noraw': lambda: render(want_raw=False),
            'render_noraw_depth': lambda: render(want_raw=False, want_depth=True, level=args.level),
            'geometry_maps_no_normals': lambda: geomaps.geometry_maps(net, batch, level=args.level, h=args.h, normals=False),
            'geometry_maps': lambda: geomaps.geometry_maps(net, batch, level=args.level, h=args.h, normals=True),
        }
        ms = {k: [] for k in variants}
        for r in range(args.warmup + args.runs):
            for k, fn in variants.items():          # interleaved: every round runs every variant once
                t, out = timed(fn, st)
                if r >= args.warmup:
                    ms[k].append(t)
        maps = out
        geo = render(want_raw=False, want_depth=True, level=args.level)
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {'res': args.res, 'samples': S, 'level': args.level, 'h': args.h, 'rays': int(ro.shape[0]), 'survivors': int(full['stats'][0]),
           'rays_crossing': int((geo['surf_index'] >= 0).sum()), 'normals': int(maps['surf_mask'].sum()), 'runs': args.runs,
           'ms_median': {k: round(v, 4) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
           'depth_pass_ms': {'with_raw': round(med['render_raw_depth'] - med['render_raw'], 4),
                             'without_raw': round(med['render_noraw_depth'] - med['render_noraw'], 4)},
           'normals_ms': round(med['geometry_maps'] - med['geometry_maps_no_normals'], 4),
           'device': torch.cuda.get_device_name(0)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
