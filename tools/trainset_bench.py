"""What feeding the training loop costs (profiles/device_batches.md): driver.train on the bench model at the configs[3] shape (inb_lan.yaml:
64 x 64 patches x 64 samples) in ONE process, with each of four feeds over the same resident synthetic sequence and the SAME sequence of window draws
(the pool of A holds every batch of the run, formed before the loop starts):

  A  pool       batches built before the loop and kept on the device (what tools/train_lan_full.py and bench.py --train do)
  B  prefetch2  invr.trainset.TrainSet.batch_fn(prefetch=2): formed on the device, two batches ahead on the set's own stream
  C  prefetch0  the same with prefetch=0: draw, launch, wait for the count, train
  D  host       the NumPy restatement of the path (tests/patch_reference.py) + .to(device) of the whole dict per iteration: a host-fed loop
                at its best, without image I/O

Prints one JSON line with the ms per batch of each feed alone (no training, host clock) and the ms per iteration of each feed (--feeds picks some, in the order given; A is usually run first and last to
show the drift of the box).  --feeds B --iters 40 is the run to put under `rocprofv3 --kernel-trace --stats` for the time of
k_patch_batch alone.

--mode plain runs the same four feeds on the plain branch (TrainSet mode 'plain', invr_ray_batch) at the configs[4] shape: cfg.N_rand 1024
rays x 128 samples, the plain-MSE objective.  Feed D is then tests/sample_reference.py's plain_batch, which like the reference's
sample_ray_h36m forms the whole frame's rays for every item; the same run under `rocprofv3 --kernel-trace --stats` gives k_ray_batch alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import invr  # noqa: E402,F401
from invr import driver, raysample, scene  # noqa: E402
from invr.config import make_cfg  # noqa: E402
from invr.trainer import NetworkWrapper  # noqa: E402
from invr.trainset import TrainSet  # noqa: E402
import bench  # noqa: E402
from tests import patch_reference as P  # noqa: E402  (feed D)
from tests import sample_reference as SR  # noqa: E402  (feed D, --mode plain)

SCENE_KEYS = ('A', 'big_A', 'pbw', 'pbounds', 'wbounds', 'R', 'Th', 'ppts', 'part_pts', 'part_pbw', 'lengths2', 'bounds')
SHARED_KEYS = ('tuv', 'tbounds')
NAMES = {'A': 'pool', 'B': 'prefetch2', 'C': 'prefetch0', 'D': 'host'}


def make_frames(n, res):
    """n frames of the bench body (pose_seed 0..n-1) as a host holds them: pixels, a 0 / 1 mask, the camera, the item's scene arrays."""
    frames, shared = [], None
    for f in range(n):
        b, ex = scene.make_scene(res, res, seed=0, frame=(3 + 11 * f) % 100, cam_dist=1.8, pose_seed=f)
        inside = b['mask_at_box'][0].reshape(res, res)
        msk = np.zeros((res, res), np.uint8)
        msk[inside] = b['occupancy'][0]
        img = np.zeros((res, res, 3), np.float32)
        img[inside] = b['rgb'][0]
        img[msk == 0] = 0
        bound = raysample.bound_mask(b['wbounds'][0], ex['K'], ex['Rc'], ex['Tc'], res, res)          # (feed D is timed without its cv2.fillPoly)
        frames.append(dict(img=img, msk=msk, bound=bound, K=ex['K'], R=ex['Rc'], T=ex['Tc'], scene={k: b[k][0] for k in SCENE_KEYS}, latent=(3 + 11 * f) % 100))
        shared = {k: b[k][0] for k in SHARED_KEYS}
    return frames, shared


def host_batch(frames, shared, index, rng, patch, dev, n_rand=None):
    """Feed D: the batch formed with NumPy on the host, then the whole dict copied to the device (n_rand: the plain branch)."""
    f = frames[index]
    if n_rand is not None:
        r = SR.plain_batch(f['img'], f['msk'], f['msk'], f['K'], f['R'], f['T'], f['scene']['wbounds'], n_rand, 0.5, 0.0, rng, bound=f['bound'])
        b = {k: r[k] for k in ('rgb', 'occupancy', 'coord', 'ray_o', 'ray_d', 'near', 'far', 'mask_at_box')}
        b.update(H=np.int64(f['msk'].shape[0]), W=np.int64(f['msk'].shape[1]))
        return upload(f, b, shared, dev)
    x0, y0, w, h, K32 = P.draw(f['msk'], f['msk'], f['K'], patch, rng)
    k_inv, R, T, o = P.camera(K32, f['R'], f['T'])
    r = P.patch_batch(f['img'], f['msk'], x0, y0, w, h, k_inv, R, T, o, f['scene']['wbounds'])
    n = r['count']
    b = {'rgb': r['rgb'], 'occupancy': r['occupancy'].astype(bool), 'coord': r['coord'], 'ray_o': np.broadcast_to(o.astype(np.float32), (n, 3)),
         'ray_d': r['ray_d'], 'near': r['near'], 'far': r['far'], 'mask_at_box': r['mask_at_box'].astype(bool), 'H': np.int64(h), 'W': np.int64(w)}
    return upload(f, b, shared, dev)


def upload(f, b, shared, dev):
    b.update({'frame_dim': np.array(f['latent'] / 100).astype(np.float32), 'latent_index': np.int64(f['latent']), 'bw_latent_index': np.int64(f['latent']),
              'frame_index': np.int64(f['latent']), 'cam_ind': np.int64(0)})
    b.update(shared)
    b.update(f['scene'])
    out = {}
    for k, v in b.items():
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(v)[None]))
        out[k] = t if k in driver.HOST_KEYS else t.to(dev, non_blocking=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--feeds', default='A,B,C,D,A')
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--frames', type=int, default=4)
    ap.add_argument('--res', type=int, default=512)
    ap.add_argument('--mode', default='patch', choices=('patch', 'plain'), help="plain: cfg.N_rand 1024 rays x 128 samples (configs[4])")
    ap.add_argument('--table-log2', type=int, default=None, help='debug: cap log2_hashmap_size')
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    plain = args.mode == 'plain'
    S, patch = (128, 64) if plain else (64, 64)
    n_rand = 1024 if plain else None
    kw = dict(N_samples=S, smpl_thresh=0.1, pair_loss_weight=1e-4, patch_size=patch)          # inb_lan.yaml over inb_377.yaml
    if plain:
        kw = dict(N_samples=S, N_rand=n_rand, body_sample_ratio=0.5, face_sample_ratio=0.0)      # inb_377.yaml, use_lpips off
    if args.table_log2:
        kw['table_log2'] = args.table_log2
    cfg = make_cfg(**kw)
    net = bench.build_model(cfg, dev).train()
    wrap = NetworkWrapper(net)
    opt = driver.make_optimizer(net, lr=1e-3, eps=1e-15)
    frames, shared = make_frames(args.frames, args.res)
    ts = TrainSet(net.cfg, device=dev, shared=shared)
    for f in frames:
        ts.add_frame(f['img'], f['msk'], f['K'], f['R'], f['T'], f['scene'], latent_index=f['latent'], orig_msk=f['msk'] if plain else None)
    n_it = args.warmup + args.iters
    order = np.random.RandomState(5).randint(len(frames), size=n_it)
    order = [int(i) for i in order]
    pool = list(ts.batches(order, np.random.RandomState(9), prefetch=0, mode=args.mode))          # feed A: every batch of the run, built before the loop
    rays = float(np.mean([b['ray_o'].shape[1] for b in pool]))

    def feed(which):
        rng = np.random.RandomState(9)
        if which == 'A':
            it = iter(pool)
            return lambda epoch, index: dict(next(it))
        if which in 'BC':
            return ts.batch_fn(order, rng, prefetch=2 if which == 'B' else 0, mode=args.mode)
        it = iter(order)
        return lambda epoch, index: host_batch(frames, shared, next(it), rng, patch, dev, n_rand)

    # the feed alone: host clock over args.iters batches with the device otherwise idle, one synchronise at the end
    import time
    alone = {}
    for which in sorted(set(w.strip().upper() for w in args.feeds.split(',') if w.strip())):
        fn = feed(which)
        for i in range(args.warmup):
            fn(0, i)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.iters):
            fn(0, i)
        torch.cuda.synchronize()
        alone[which] = round(1e3 * (time.perf_counter() - t0) / args.iters, 4)
        print('feed %s alone: %.4f ms per batch' % (which, alone[which]), file=sys.stderr, flush=True)

    results = []
    for which in [w.strip().upper() for w in args.feeds.split(',') if w.strip()]:
        fn = feed(which)
        driver.train(wrap, opt, fn, 1, args.warmup)
        out = driver.train(wrap, opt, fn, 1, args.iters)
        assert np.isfinite(out['losses']).all()
        print('feed %s (%s): %.4f ms per iteration' % (which, NAMES[which], 1e3 * out['seconds'] / out['iterations']), file=sys.stderr, flush=True)
        results.append({'feed': which, 'name': NAMES[which], 'ms_per_iter': round(1e3 * out['seconds'] / out['iterations'], 4),
                        'rays_per_iter': round(out['ray_samples'] / out['iterations'] / S, 1)})
    workload = ('configs[4] shape: N_rand 1024 rays x 128 samples, plain MSE' if plain else 'configs[3] shape: 64x64 patches x 64 samples') + ', bench model, driver.train'
    print(json.dumps({'workload': workload, 'mode': args.mode, 'iters': args.iters,
                      'frames': args.frames, 'res': args.res, 'mean_rays': rays, 'device': torch.cuda.get_device_name(0), 'feed_alone_ms_per_batch': alone, 'feeds': results}))


if __name__ == '__main__':
    main()
