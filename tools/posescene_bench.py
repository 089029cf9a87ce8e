"""Timing of the novel-pose path on the bench scene's full-size model (profiles/pose_scenes.md):
  kernel     invr_distance_volume alone on the posed body of frame 0 and its lattice: device events, --warmup + --runs calls, median;
  frame      PoseScenes.frame() per frame over the sequence, host wall clock per call while the stream still holds the previous frames'
             work, and the device time of one frame's whole scene build (events around the call);
  run_poses  driver.run_poses at 512 x 512 x 128 over --frames pose_seed frames with 1 and 8 frames in flight, against the same loop
             over (a) prebuilt batches and (b) prebuilt scene tensors with the rays generated per frame: what the loop could already
             do with scene tensors prepared elsewhere.  The variants alternate, --repeats times each; medians.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import invr  # noqa: E402,F401
from invr import driver, prep, scene  # noqa: E402
from invr.config import make_cfg  # noqa: E402
from invr.posescene import PoseScenes  # noqa: E402
import bench  # noqa: E402


class Prebuilt:
    """The PoseScenes interface over frames (and, with batches=True, whole eval batches) built ahead of the timed loop."""
    def __init__(self, scenes, frames, camera, batches):
        self.device, self.scenes = scenes.device, scenes
        self.frames = [scenes.frame(**kw) for kw in frames]
        self.batches = [scenes.eval_batch(f, *camera) for f in self.frames] if batches else None
        self.i = 0

    def frame(self, **kw):
        self.i += 1
        return self.i - 1

    def eval_batch(self, i, *camera):
        return dict(self.batches[i]) if self.batches is not None else self.scenes.eval_batch(self.frames[i], *camera)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=20)
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--samples', type=int, default=128)
    ap.add_argument('--table-log2', type=int, default=None, help='debug: cap log2_hashmap_size')
    args = ap.parse_args()
    dev = 'cuda:0'
    cfg = make_cfg(N_samples=args.samples, **({'table_log2': args.table_log2} if args.table_log2 else {}))
    net = bench.build_model(cfg, dev)
    H = W = args.size
    f = 555.0 * H / 512.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1]], dtype=np.float64)          # scene.make_scene's camera at this size
    frames, scenes, camera = [], None, None
    for k in range(args.frames):
        b, e = scene.make_scene(8, 8, seed=0, frame=3, cam_dist=1.8, pose_seed=k)          # the bench sequence's bodies (the rays are made here)
        if scenes is None:
            big = np.zeros(72)
            big[5], big[8] = np.deg2rad(30), np.deg2rad(-30)
            scenes = PoseScenes(scene._J, scene.PARENTS, e['weights'], e['parts'], e['tpose'], b['tuv'][0], b['tbounds'][0], big, cfg=cfg, device=dev)
            camera = (H, W, K, e['Rc'], e['Tc'])
        frames.append(dict(wxyz=e['wpts'], Th=b['Th'][0], poses=e['poses'], latent_index=3, R=b['R'][0]))
    out = {'frames': args.frames, 'size': [H, W, args.samples]}
    st = torch.cuda.current_stream()

    # ---- the kernel alone
    f0 = scenes.frame(**frames[0])
    origin, step, dims = f0.host['origin'], f0.host['step'], f0.host['dims']
    ms = []
    for i in range(args.warmup + args.runs):
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        prep.distance_volume(f0['ppts'], origin, step, dims)
        b_.record(st)
        b_.synchronize()
        ms.append(a.elapsed_time(b_))
    out['kernel'] = {'dims': list(dims), 'points': int(np.prod(dims)), 'vertices': int(f0['ppts'].shape[0]),
                     'ms_median': statistics.median(ms[args.warmup:]), 'ms_min': min(ms[args.warmup:]), 'ms_max': max(ms[args.warmup:])}

    # ---- frame(): host time per call with the stream busy, device time of one whole scene build
    host, devms = [], []
    for rep in range(2):
        torch.cuda.synchronize()
        keep, host = [], []
        for kw in frames:
            t = time.perf_counter()
            keep.append(scenes.frame(**kw))
            host.append((time.perf_counter() - t) * 1e3)
        torch.cuda.synchronize()
    for kw in frames:
        a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        scenes.frame(**kw)
        b_.record(st)
        b_.synchronize()
        devms.append(a.elapsed_time(b_))
    out['frame'] = {'host_ms_median': statistics.median(host), 'host_ms_max': max(host), 'device_ms_median': statistics.median(devms),
                    'points_per_frame': [int(np.prod(k.host['dims'])) for k in keep]}
    del keep

    # ---- run_poses against the prebuilt loops
    from invr.renderer import Renderer

    def timed(make, lanes, renderer):
        s = make()
        torch.cuda.synchronize()
        t = time.perf_counter()
        driver.run_poses(net, s, frames, camera, in_flight=lanes, on_frame=lambda i, img, acc: None, renderer=renderer)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3 / len(frames)

    variants = {'run_poses': lambda: scenes, 'prebuilt_batches': lambda: Prebuilt(scenes, frames, camera, True),
                'prebuilt_scenes': lambda: Prebuilt(scenes, frames, camera, False)}
    res = {}
    for lanes in (1, 8):
        renderer = Renderer(net)          # one for all runs of this lane count: the lanes' workspaces and the survivor bound stay
        for _ in range(2):
            timed(variants['run_poses'], lanes, renderer)                    # warm: lanes, workspaces, the survivor bound
        ms = {k: [] for k in variants}
        for rep in range(args.repeats):
            for k, make in variants.items():
                ms[k].append(timed(make, lanes, renderer))
        renderer.flush(release=True)
        del renderer
        torch.cuda.empty_cache()
        med = {k: statistics.median(v) for k, v in ms.items()}
        res['in_flight_%d' % lanes] = {'ms_per_frame_median': med, 'ms_per_frame_all': {k: [round(x, 4) for x in v] for k, v in ms.items()},
                                       'ratio_to_prebuilt_batches': med['run_poses'] / med['prebuilt_batches'],
                                       'ratio_to_prebuilt_scenes': med['run_poses'] / med['prebuilt_scenes']}
    out['run_poses'] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
