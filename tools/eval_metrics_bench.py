"""Cost of the on-device evaluation metrics (profiles/eval_metrics.md), on the bench's 512 x 512 x 128 sequence:
  loop     (a) ms per frame of driver.run_evaluate with metrics='host' and metrics='device', in_flight = 8, median of the passes after
           a warm-up; (c) ms per rendered frame of the same loop with no evaluator in it (outputs on the device, frames only joined).
           A pass is 160 frames; its figure is the steady-state interval between the moments the loop asks for frame 16 and for the
           last frame (the lanes' workspaces are allocated during the first frames of every pass: seconds, in some allocator states)
  kernels  a short device-metrics run for `rocprofv3 --kernel-trace --stats -- python tools/eval_metrics_bench.py kernels`  (b)
  frame    the evaluator alone on one assembled 512 x 512 frame: ms per evaluate() over 200 calls (launch-bound or not)"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from invr import driver  # noqa: E402
from invr.config import make_cfg  # noqa: E402
from invr.evaluator import Evaluator  # noqa: E402
from invr.renderer import Renderer  # noqa: E402


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else 'loop'
    passes = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = torch.device('cuda', 0)
    cfg = make_cfg(N_samples=128)
    net = bench.build_model(cfg, dev)
    cpu, gpu = bench.frame_batches(512, 1.8, 10, dev)
    # device-resident batches (as bench.py renders them) whose H / W / index scalars stay host tensors, as a data loader delivers them
    batches = [dict(g, **{k: c[k] for k in driver.HOST_KEYS if k in c}) for c, g in zip(cpu, gpu)]
    seq = batches * 16                                                    # 160 frames per pass
    SKIP = 16
    stamps = []

    def stamped():
        del stamps[:]
        for b in seq:
            stamps.append(time.perf_counter())
            yield b
    r = Renderer(net)

    def render_only():
        from collections import deque
        r.in_flight, r.eval_to_cpu = 8, False
        q = deque()
        for b in stamped():
            with torch.no_grad():
                q.append(r.render(dict(b)))
            while len(q) >= 8:
                q.popleft()['rgb_map']
        while q:
            q.popleft()['rgb_map']
        torch.cuda.synchronize()
        r.in_flight, r.eval_to_cpu = 1, True
        r.flush(release=True)
        r._cap_hint = None

    def timed(fn):
        torch.cuda.synchronize()
        out = fn()
        torch.cuda.synchronize()
        return (stamps[-1] - stamps[SKIP]) / (len(stamps) - 1 - SKIP) * 1e3, out

    if mode == 'kernels':
        driver.run_evaluate(net, seq[:40], device=dev, in_flight=8, renderer=r, metrics='device')
        out = driver.run_evaluate(net, seq[:10], device=dev, in_flight=8, renderer=r, metrics='device')
        print('psnr', out['psnr'][:3], 'ssim', out['ssim'][:3])
        return
    if mode == 'frame':
        ev = Evaluator(cfg={'test_full': True, 'fast_eval': True, 'result_dir': ''})
        b = batches[0]
        with torch.no_grad():
            ret = {'rgb_map': Renderer(net).render(dict(b))['rgb_map'].to(dev)}
        for n in (20, 200):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                ev.evaluate(ret, b)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            print('evaluate() x %d: host %.3f ms per call, with the device drained %.3f ms per call' % (n, (t1 - t0) / n * 1e3, (t2 - t0) / n * 1e3))
        ev.collect()
        return
    # a renderer of its own per pass for each (run_evaluate's default: lanes created, the first frame joined at once, lanes released)
    host = lambda: driver.run_evaluate(net, stamped(), device=dev, in_flight=8)
    devm = lambda: driver.run_evaluate(net, stamped(), device=dev, in_flight=8, metrics='device')
    res = {'host': [], 'device': [], 'render_only': []}
    for p in range(passes + 2):                                          # two warm-up passes, then interleaved
        for name, fn in (('host', host), ('device', devm), ('render_only', render_only)):
            ms, out = timed(fn)
            if p >= 2:
                res[name].append(ms)
            if p == 0 and out is not None:
                print(name, 'psnr[0..2]', ['%.12f' % v for v in out['psnr'][:3]], 'ssim', ['%.12f' % v for v in out.get('ssim', [])[:3]], flush=True)
    for name, v in res.items():
        print('%-12s ms per frame: median %.3f  min %.3f  max %.3f  (%d passes of %d frames)' % (name, statistics.median(v), min(v), max(v), len(v), len(seq) - 1 - SKIP), flush=True)
    print('reserved GB %.1f' % (torch.cuda.memory_reserved() / 1e9))


if __name__ == '__main__':
    main()
