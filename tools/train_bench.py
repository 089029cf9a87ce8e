"""Training-iteration timing on one MI355X (BASELINE configs[4] shape by default: 1024 rays x 128 samples, full-size model).
  python tools/train_bench.py [--rays-side 32] [--samples 128] [--iters 50] [--graph] [--prof]
Reports the un-synchronised iteration time (the loop only syncs at the end) and a synchronised fwd / bwd / opt split.
  python tools/train_bench.py --lpips [--iters 50]
The same iteration with cfg.use_lpips True (the configs/inb/inb_377.yaml default) and a seeded PerceptualLoss(allow_random=True) at a
64 x 64 and a 56 x 56 patch: cfg.fused_perceptual False (torch ops) against True (csrc/k_perceptual.hip), interleaved in one process,
then the per-launch device times of the perceptual kernels (profiles/perceptual_loss.md).
  python tools/train_bench.py --ssim | --tv [--iters 50]
The same iteration with cfg.use_ssim / cfg.use_tv_image True at a 64 x 64 patch: the plain-MSE iteration, cfg.fused_image_terms False
(torch ops) and True (csrc/k_imgloss.hip), interleaved in one process, then the launches per iteration (profiles/image_terms.md)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import invr  # noqa: E402,F401
from invr import scene, driver  # noqa: E402
from invr.config import make_cfg  # noqa: E402
from invr.network import Network  # noqa: E402
from invr.trainer import NetworkWrapper  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--rays-side', type=int, default=32)
ap.add_argument('--samples', type=int, default=128)
ap.add_argument('--iters', type=int, default=50)
ap.add_argument('--graph', action='store_true', help='op-by-op autograd graph (cfg.train_fused False)')
ap.add_argument('--torch-adam', action='store_true')
ap.add_argument('--prof', action='store_true')
ap.add_argument('--thresh', type=float, default=0.05)
ap.add_argument('--lpips', action='store_true', help='A/B of the use_lpips iteration: cfg.fused_perceptual False against True')
ap.add_argument('--ssim', action='store_true', help='A/B of the use_ssim iteration: cfg.fused_image_terms False against True, next to plain MSE')
ap.add_argument('--tv', action='store_true', help='the same for use_tv_image')
args = ap.parse_args()
DEV = 'cuda:0'
cfg = make_cfg(N_samples=args.samples, smpl_thresh=args.thresh)
cfg.train_fused = not args.graph
with torch.device(DEV):
    net = Network(cfg=cfg)
net = net.to(DEV).train()
g = torch.Generator(device=DEV).manual_seed(0)
with torch.no_grad():
    for name, p in net.named_parameters():
        if name.endswith('embedder.dense') or name.endswith('embedder.hash'):
            p.normal_(0.0, 0.1, generator=g)


def patch(s):
    bnp, _ = scene.make_scene(512, 512, seed=0, cam_dist=1.8, crop=(256 - s // 2, 256 - s // 2, s, s))
    return {k: v.to(DEV) for k, v in scene.to_torch(bnp).items()}


def lpips_ab():
    from invr.losses import PerceptualLoss
    torch.manual_seed(0)
    net.cfg.use_lpips = True
    wrap = NetworkWrapper(net, perceptual_loss=PerceptualLoss(allow_random=True))
    opt = driver.make_optimizer(net, fused=not args.torch_adam)
    it = 0
    for side in (64, 56):
        gb = patch(side)
        ms = {False: [], True: []}
        for rep in range(3):                               # interleaved: drift of the box shows as spread within an arm
            for fused in (False, True):
                net.cfg.fused_perceptual = fused
                for _ in range(5):
                    it += 1
                    gb['iter_step'] = it + 1
                    loss = driver.train_step(wrap, opt, gb, it + 1)[0]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    it += 1
                    gb['iter_step'] = it + 1
                    loss = driver.train_step(wrap, opt, gb, it + 1)[0]
                torch.cuda.synchronize()
                ms[fused].append((time.perf_counter() - t0) / args.iters * 1e3)
        a, b = np.array(ms[False]), np.array(ms[True])
        print('use_lpips %dx%d patch, %d rays x %d samples: fused_perceptual False %s ms (median %.3f), True %s ms (median %.3f), ratio %.3f, loss %.5f'
              % (side, side, gb['ray_o'].shape[1], args.samples, np.round(a, 3).tolist(), np.median(a), np.round(b, 3).tolist(), np.median(b),
                 np.median(b) / np.median(a), float(loss)))
        from torch.profiler import profile, ProfilerActivity
        for fused in (False, True):
            net.cfg.fused_perceptual = fused
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    it += 1
                    gb['iter_step'] = it + 1
                    driver.train_step(wrap, opt, gb, it + 1)
                torch.cuda.synchronize()
            ev = [e for e in prof.key_averages() if e.device_time_total > 0]
            print('  fused_perceptual %s: %d device launches per iteration, %.1f us of device time per iteration'
                  % (fused, sum(e.count for e in ev) // 5, sum(e.device_time_total for e in ev) / 5))
            if fused:
                for e in sorted(ev, key=lambda e: -e.device_time_total):
                    if 'k_perc' in e.key or 'lpips' in e.key:
                        print('    %-90s x%d per iteration  %.1f us each' % (e.key[:90], e.count // 5, e.device_time_total / e.count))


def image_term_ab(flag):
    torch.manual_seed(0)
    setattr(net.cfg, flag, True)
    net.cfg.builtin_image_terms = True
    wrap = NetworkWrapper(net)                              # builds invr.losses.SSIM / TVImageLoss
    opt = driver.make_optimizer(net, fused=not args.torch_adam)
    gb = patch(64)
    gb['H'], gb['W'] = gb['H'].cpu(), gb['W'].cpu()          # as TrainSet hands them: host tensors, no read-back per iteration
    arms = (('mse', False, True), ('torch ops', True, False), ('fused', True, True))
    ms = {a[0]: [] for a in arms}
    it = 0
    for rep in range(3):                                   # interleaved: drift of the box shows as spread within an arm
        for name, on, fused in arms:
            setattr(net.cfg, flag, on)
            net.cfg.fused_image_terms = fused
            for _ in range(5):
                it += 1
                gb['iter_step'] = it + 1
                loss = driver.train_step(wrap, opt, gb, it + 1)[0]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                it += 1
                gb['iter_step'] = it + 1
                loss = driver.train_step(wrap, opt, gb, it + 1)[0]
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) / args.iters * 1e3)
    print('%s 64x64 patch, %d rays x %d samples, ms per iteration: %s   last loss %.5f'
          % (flag, gb['ray_o'].shape[1], args.samples,
             '   '.join('%s %s (median %.3f)' % (k, np.round(v, 3).tolist(), np.median(v)) for k, v in ms.items()), float(loss)))
    from torch.profiler import profile, ProfilerActivity
    for name, on, fused in arms:
        setattr(net.cfg, flag, on)
        net.cfg.fused_image_terms = fused
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                it += 1
                gb['iter_step'] = it + 1
                driver.train_step(wrap, opt, gb, it + 1)
            torch.cuda.synchronize()
        ev = [e for e in prof.key_averages() if e.device_time_total > 0]
        print('  %-9s: %d device launches per iteration, %.1f us of device time per iteration'
              % (name, sum(e.count for e in ev) // 5, sum(e.device_time_total for e in ev) / 5))
        if fused and on:
            for e in sorted(ev, key=lambda e: -e.device_time_total):
                if any(k in e.key for k in ('k_ssim', 'k_tv', 'k_imgloss', 'k_train_loss_term', 'k_perc_assemble')):
                    print('    %-90s x%d per iteration  %.1f us each' % (e.key[:90], e.count // 5, e.device_time_total / e.count))


if args.lpips:
    lpips_ab()
    sys.exit(0)
if args.ssim or args.tv:
    image_term_ab('use_ssim' if args.ssim else 'use_tv_image')
    sys.exit(0)
s = args.rays_side
gb = patch(s)
print('patch rays', gb['ray_o'].shape[1], 'samples', args.samples)
wrap = NetworkWrapper(net)
opt = driver.make_optimizer(net, fused=not args.torch_adam)


def step(i, timing=None):
    gb['iter_step'] = i + 2
    if timing is None:
        return driver.train_step(wrap, opt, gb, i + 2)[0]
    t0 = time.perf_counter()
    ret, loss, stats, _ = wrap(gb, split='train'); loss = loss.mean(); torch.cuda.synchronize(); t1 = time.perf_counter()
    opt.zero_grad(set_to_none=True); loss.backward(); torch.cuda.synchronize(); t2 = time.perf_counter()
    opt.step(); torch.cuda.synchronize(); t3 = time.perf_counter()
    timing.append((t1 - t0, t2 - t1, t3 - t2))
    return loss.detach()


for i in range(5):
    l = step(i)
torch.cuda.synchronize()
t0 = time.perf_counter()
for i in range(args.iters):
    l = step(i + 5)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / args.iters
print('iteration %.3f ms (un-synchronised loop), %.3e ray-samples/s, loss %.5f' % (dt * 1e3, gb['ray_o'].shape[1] * args.samples / dt, float(l)))
T = []
for i in range(10):
    step(100 + i, T)
T = np.array(T) * 1e3
print('synchronised fwd / bwd / opt ms', T.mean(0), 'sum', T.sum(1).mean())
print('stats', wrap.renderer.last_stats.cpu().numpy()[:15])
if args.prof:
    from torch.profiler import profile, ProfilerActivity
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for i in range(5):
            step(200 + i)
        torch.cuda.synchronize()
    print(prof.key_averages().table(sort_by='cuda_time_total', row_limit=40, max_name_column_width=70))
if os.environ.get('HOSTPROF'):
    # host side of the loop: time to ISSUE n iterations (no synchronisation inside) vs time until the GPU has finished them, and a cProfile
    # of the issuing thread
    import cProfile, pstats, io
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(40):
        step(300 + i)
    t_issue = time.perf_counter() - t0
    torch.cuda.synchronize()
    t_done = time.perf_counter() - t0
    print('40 iterations: issued in %.3f ms each, finished in %.3f ms each' % (t_issue / 40 * 1e3, t_done / 40 * 1e3))
    pr = cProfile.Profile()
    pr.enable()
    for i in range(40):
        step(400 + i)
    pr.disable()
    torch.cuda.synchronize()
    s = io.StringIO()
    pstats.Stats(pr, stream=s).sort_stats('cumulative').print_stats(45)
    print(s.getvalue()[:9000])
