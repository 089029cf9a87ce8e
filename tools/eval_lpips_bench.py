"""Cost of the evaluator's LPIPS on the device (profiles/eval_lpips.md), with LpipsVgg.random weights at 512 x 512 and 1024 x 1024:
  kernels  ms per frame of invr_lpips_fwd (keep = 0: LpipsVgg.__call__), interleaved in ONE process with the same network written as
           torch ops (F.conv2d / max_pool2d, fp32, the distance as the lpips package writes it) on the same GPU.  The torch path is
           timed after its warm-up; the time of its first call (MIOpen's search for 13 shapes) is reported separately.  Each figure
           comes with the fraction of the exact-fp32 matrix floor (155 TFLOP/s measured) it reaches: 2 x 2 x MACs / 155e12 / time.
  loop     frames per second of driver.run_evaluate(metrics='device') on the bench's 512 x 512 x 128 sequence without and with the
           metric.
usage: python tools/eval_lpips_bench.py [kernels|loop|all] [--no-torch] [--sizes 512,1024]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invr import lpips_eval  # noqa: E402

PEAK = 155e12
BLOCK = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)


def macs_per_image(H, W):
    return sum(9 * i * o * (H >> b) * (W >> b) for i, o, b in zip(lpips_eval.CIN, lpips_eval.COUT, BLOCK))


def torch_lpips(weights, shift, scale, a, b):
    """The network as torch ops: a, b (H, W, 3) device images -> the 0-dim value"""
    conv_w, conv_b, lin_w = weights
    x = torch.stack([a, b]).permute(0, 3, 1, 2)
    x = (x - shift) / scale
    val = 0
    for l in range(13):
        if l > 0 and BLOCK[l] != BLOCK[l - 1]:
            x = F.max_pool2d(x, 2, 2)
        x = F.relu(F.conv2d(x, conv_w[l], conv_b[l], padding=1))
        if l in lpips_eval.TAPS:
            n = x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + 1e-10)
            d = (n[0:1] - n[1:2]) ** 2
            val = val + (d * lin_w[lpips_eval.TAPS.index(l)].reshape(1, -1, 1, 1)).sum(1, keepdim=True).mean([2, 3], keepdim=True)
    return val.reshape(())


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def kernels(sizes, with_torch):
    dev = torch.device('cuda', 0)
    cpu = lpips_eval.random_tensors(0)
    net = lpips_eval.LpipsVgg.from_tensors(*cpu, device=dev)
    tw = [[t.to(dev) for t in ts] for ts in cpu]
    shift = torch.tensor(lpips_eval.SHIFT, device=dev).reshape(1, 3, 1, 1)
    scale = torch.tensor(lpips_eval.SCALE, device=dev).reshape(1, 3, 1, 1)
    for S in sizes:
        g = torch.Generator().manual_seed(S)
        a = torch.rand(S, S, 3, generator=g).to(dev)
        b = (a + 0.05 * torch.randn(S, S, 3, generator=g).to(dev)).clamp(0, 1)
        flop = 2.0 * 2.0 * macs_per_image(S, S)
        hip = lambda: net(a, b)
        v_hip = float(hip().cpu())
        timed(hip, 2)
        n = 10 if S <= 512 else 4
        first = timed(hip, n)
        print('%d x %d: %.1f GFLOP per frame, floor %.3f ms' % (S, S, flop / 1e9, flop / PEAK * 1e3), flush=True)
        print('  hip   (before the torch path ran)   %.3f ms per frame   %.1f %% of the floor   value %.9g' % (first, flop / PEAK * 1e5 / first, v_hip), flush=True)
        if not with_torch:
            continue
        tor = lambda: torch_lpips(tw, shift, scale, a, b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            v_t = float(tor().cpu())
        print('  torch first call                    %.1f ms   value %.9g' % ((time.perf_counter() - t0) * 1e3, v_t), flush=True)
        with torch.no_grad():
            timed(tor, 2)
            res = {'hip': [], 'torch': []}
            for _ in range(3):                                             # interleaved rounds
                res['hip'].append(timed(hip, n))
                res['torch'].append(timed(tor, n))
        for k in ('hip', 'torch'):
            m = statistics.median(res[k])
            print('  %-5s interleaved, median of 3 x %d   %.3f ms per frame (min %.3f max %.3f)   %.1f %% of the floor'
                  % (k, n, m, min(res[k]), max(res[k]), flop / PEAK * 1e5 / m), flush=True)
        print('  reserved GB %.2f' % (torch.cuda.memory_reserved() / 1e9), flush=True)


def loop():
    import bench
    from invr import driver
    from invr.config import make_cfg
    from invr.evaluator import Evaluator
    dev = torch.device('cuda', 0)
    cfg = make_cfg(N_samples=128)
    net = bench.build_model(cfg, dev)
    cpu, gpu = bench.frame_batches(512, 1.8, 10, dev)
    batches = [dict(g, **{k: c[k] for k in driver.HOST_KEYS if k in c}) for c, g in zip(cpu, gpu)]
    seq = batches * 8
    lp = lpips_eval.LpipsVgg.random(0, device=dev)
    ecfg = {'test_full': True, 'fast_eval': True, 'dry_run': False, 'eval_part': '', 'result_dir': '', 'eval_fused_lpips': True}
    sys.modules.setdefault('lpips', None)                                  # 'without': no weights anywhere, whatever this host has installed
    res = {'without': [], 'with': []}
    for p in range(4):                                                     # one warm-up pass, then interleaved
        for name in ('without', 'with'):
            ev = Evaluator(cfg=dict(ecfg), lpips=lp if name == 'with' else None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = driver.run_evaluate(net, seq, device=dev, in_flight=8, metrics='device', evaluator=ev)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if p > 0:
                res[name].append(len(seq) / dt)
            elif name == 'with':
                print('lpips[0..2]', ['%.9g' % v for v in out['lpips'][:3]], flush=True)
    for name, v in res.items():
        print('run_evaluate(metrics=device) %-8s lpips: %.1f frames per second (median of %d passes of %d frames; min %.1f max %.1f)'
              % (name, statistics.median(v), len(v), len(seq), min(v), max(v)), flush=True)


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('mode', nargs='?', default='all', choices=('kernels', 'loop', 'all'))
    ap.add_argument('--no-torch', action='store_true', help='kernels: time the HIP path only')
    ap.add_argument('--sizes', default='512,1024', help='kernels: comma-separated frame sides')
    args = ap.parse_args()
    if args.mode in ('kernels', 'all'):
        kernels([int(v) for v in args.sizes.split(',')], not args.no_torch)
    if args.mode in ('loop', 'all'):
        loop()


if __name__ == '__main__':
    main()
