"""GPU: the pair lists k_deform_pairs leaves behind now that it warps each pair itself (csrc/k_warp.hip: lane j of a wave's 64-pair
batch computes the canonical point and view direction of its own pair, then the wave runs the deformer on the batch).

`invr_geometry_fwd` is driven with a caller-owned workspace filled with bytes of 0x7F, and `_abi.ws_views` is read afterwards, on a
small scene (2^12-row tables, a crop of a 64 x 64 frame, 32 samples per ray, windows of its ray list):

  1. boundary counts — ray windows chosen from the per-ray pair counts of the whole crop so that some part's list count (the
     far-constant pair included) is exactly 1, in 2..63, 64, 65, in 255..257, and above 256 without being a multiple of 64: a batch
     with one live lane, a partial batch, a full one, one lane into the second batch of a wave, the workgroup's edge (256 lanes) and
     a ragged last batch of a later workgroup.  The test asserts that every class was hit;
  2. values — canonical point and direction within 1e-5 of the dense `stages.warp_deform`, the residual against `net.resd` on the
     SAME canonical point (above 2e-6 for less than a 1e-4 fraction of a list, never above 1e-3), |l_r| <= 0.05 + 1e-7, and the
     far-constant pair exactly zero: the bounds of test_gpu_production_kernels.py's whole-frame test;
  3. nothing past the list — entries [count, lcap) of l_x / l_d / l_r still hold the fill (lanes clamped to the last pair store nothing);
  4. placement independence — the same rays as one call and as two calls: every listed (ray-sample, part) has identical bits;
  5. (GPU only) a 256 x 256 x 128 frame of the bench scene: more than 131,072 pairs in a part, so that a workgroup of the capped
     grid (512 workgroups x 256 lanes) walks a second batch; checks 2 and 3 on it.

tests/test_hostsim_warp_in_deformer_cpu.py runs cases 1-4 through the host build of the kernel sources."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from invr import _abi, params, scene, stages          # noqa: E402
from invr.config import make_cfg                        # noqa: E402
from invr.network import Network                        # noqa: E402

DEV = 'cuda:0'
S = 32
FRAME = dict(H=64, W=64, seed=0, cam_dist=1.8, crop=(8, 8, 48, 48))
FILL = 0x7F
FILL32 = 0x7F7F7F7F
GRID_CAP = 512 * 256            # launch_warp_pairs: workgroups x lanes of one sweep over a part's list

_CACHE = {}


def world(frame=None, samples=S):
    """(net, ctx, rays) of a frame on DEV, built once per device and frame."""
    key = (DEV, samples, tuple(sorted((frame or FRAME).items())))
    if key not in _CACHE:
        cfg = make_cfg(table_log2=12, N_samples=samples)
        net = Network(cfg=cfg)
        net.load_state_dict(params.init_state_dict(cfg, seed=3), strict=True)
        net = net.to(DEV).eval()
        bnp, _ = scene.make_scene(**(frame or FRAME))
        gb = {k: v.to(DEV) for k, v in scene.to_torch(bnp).items()}
        ctx = net.prepare(gb)
        _CACHE[key] = (net, ctx, tuple(gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far')))
    return _CACHE[key]


def geometry(net, ctx, rays, samples=S, max_active=0):
    """invr_geometry_fwd on a ray list with a workspace of this call's own, every byte 0x7F on entry -> (stats, views)."""
    ro, rd, nr, fa = (r.contiguous() for r in rays)
    n = ro.shape[0]
    nbytes = _abi.lib().invr_workspace_bytes(n, samples, max_active)
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    ws = raw[off:off + nbytes]
    ws.fill_(FILL)
    net._ws = ws                                    # Network.workspace hands out a buffer that is large enough as it is
    try:
        out = net.geometry_pass(ctx, ro, rd, nr, fa, samples, max_active=max_active)
        torch.cuda.synchronize()
    finally:
        net._ws = None
    assert out['_ws'][0].data_ptr() == ws.data_ptr()
    st = out['stats'].cpu().numpy()
    assert st[6] == 0
    return st, _abi.ws_views(*out['_ws'])


def check_lists(net, ctx, rays, st, v, samples=S):
    """Checks 2 and 3 on one call's lists -> the five list counts."""
    ro, rd, nr, fa = rays
    Na, lc = int(st[0]), v['lcap']
    counts = [int(st[1 + p]) for p in range(5)]
    assert min(counts) >= 1
    for p in range(5):
        c = counts[p]
        # 3. nothing past the list
        for k in ('l_x', 'l_d', 'l_r'):
            tail = v[k][p].view(torch.int32)[:, c:]
            assert tail.shape[1] == lc - c and bool((tail == FILL32).all()), (k, p, c)
        # 2. the far-constant pair: zero weights -> canonical origin, zero direction
        x0 = v['l_x'][p][:, c - 1] - v['l_r'][p][:, c - 1]
        assert float(x0.abs().max()) == 0.0 and float(v['l_d'][p][:, c - 1].abs().max()) == 0.0, p
    if Na == 0:
        assert max(counts) == 1
        return counts
    act = v['active_idx'][:Na]
    pts, dirs = stages.pose_points(ctx.scene, ro.contiguous(), rd.contiguous(), nr.contiguous(), fa.contiguous(), samples, act)
    bw, _ = stages.knn_blend(ctx.scene, pts)
    pf = v['pflags'][:Na].int()
    flag = torch.stack([((pf >> p) & 1) for p in range(5)], 1).to(torch.uint8)
    tp, td, rs = stages.warp_deform(ctx.scene, ctx.model, pts, dirs, bw, flag)
    for p in range(5):
        cnt = counts[p] - 1
        assert cnt == int(flag[:, p].sum())
        if cnt == 0:
            continue
        slots = v['l_slot'][p][:cnt].long()
        r = v['l_r'][p][:, :cnt].t().contiguous()
        xb = (v['l_x'][p][:, :cnt].t() - r).contiguous()                           # init_bigpose (l_x = init_bigpose + resd)
        d = v['l_d'][p][:, :cnt].t()
        ex = (xb - (tp[slots, p] - rs[slots, p])).abs().max(1)[0]
        ed = (d - td[slots, p]).abs().max(1)[0]
        er = (r - net.resd(xb[None], ctx)[0]).abs().max(1)[0]
        fr = float((er > 2e-6).float().mean())
        print('part %d: %d pairs, |dx| %.2e |dd| %.2e |dr| %.2e (%.1e above 2e-6)' % (p, cnt, float(ex.max()), float(ed.max()), float(er.max()), fr))
        assert float(ex.max()) < 1e-5 and float(ed.max()) < 1e-5, (p, cnt, float(ex.max()), float(ed.max()))
        assert fr < 1e-4 and float(er.max()) < 1e-3, (p, cnt, float(er.max()), fr)
        assert float(r.abs().max()) <= 0.05 + 1e-7
    return counts


def per_ray_pairs(st, v, n, samples=S):
    """(5, n): listed pairs of every ray and part of a call."""
    Na = int(st[0])
    ray = (v['active_idx'][:Na].long() // samples).cpu().numpy()
    pf = v['pflags'][:Na].cpu().numpy()
    return np.stack([np.bincount(ray[((pf >> p) & 1) == 1], minlength=n) for p in range(5)])


def find_window(per_ray, lo, hi):
    """A window [r0, r1) of the ray list in which some part lists lo-1 .. hi-1 pairs (its count then includes the far-constant pair)."""
    n = per_ray.shape[1]
    for p in range(5):
        cum = np.concatenate([[0], np.cumsum(per_ray[p])])
        for r0 in range(n):
            r1 = max(r0 + 1, int(np.searchsorted(cum, cum[r0] + lo - 1, 'left')))
            if r1 <= n and lo - 1 <= cum[r1] - cum[r0] <= hi - 1:
                return r0, r1
    return None


CLASSES = [('1', lambda c: c == 1), ('2..63', lambda c: 2 <= c <= 63), ('64', lambda c: c == 64), ('65', lambda c: c == 65),
           ('255..257', lambda c: 255 <= c <= 257), ('>256, not a multiple of 64', lambda c: c > 256 and c % 64 != 0)]


def test_boundary_counts_values_and_fill():
    net, ctx, rays = world()
    n = rays[0].shape[0]
    st, v = geometry(net, ctx, rays)
    per_ray = per_ray_pairs(st, v, n)
    seen = check_lists(net, ctx, rays, st, v)                    # the whole crop: several workgroups per part
    assert max(seen) > 1024
    windows = [find_window(per_ray, lo, hi) for lo, hi in ((1, 1), (2, 63), (64, 64), (65, 65), (255, 257), (300, 319))]
    assert all(w is not None for w in windows), windows
    for r0, r1 in windows:
        sub = tuple(r[r0:r1] for r in rays)
        st, v = geometry(net, ctx, sub)
        counts = check_lists(net, ctx, sub, st, v)
        print('rays [%d, %d): list counts %s' % (r0, r1, counts))
        seen += counts
    for name, hit in CLASSES:
        assert any(hit(c) for c in seen), (name, sorted(set(seen)))


def listed_bits(st, v, ray0, samples=S):
    """{part: (keys, bits)}: ray-sample index of every listed pair (in the numbering of the whole ray list) and the bits of its
    l_x / l_d / l_r entries, sorted by key."""
    out = {}
    act = v['active_idx'].long()
    for p in range(5):
        cnt = int(st[1 + p]) - 1
        key = act[v['l_slot'][p][:cnt].long()] + ray0 * samples
        bits = torch.cat([v[k][p].view(torch.int32)[:, :cnt] for k in ('l_x', 'l_d', 'l_r')], 0)
        o = key.argsort()
        out[p] = (key[o].clone(), bits[:, o].clone())
    return out


def test_placement_independence_bit_for_bit():
    net, ctx, rays = world()
    n = rays[0].shape[0]
    whole = listed_bits(*geometry(net, ctx, rays), 0)
    h = n // 2 + 1
    a = listed_bits(*geometry(net, ctx, tuple(r[:h] for r in rays)), 0)
    b = listed_bits(*geometry(net, ctx, tuple(r[h:] for r in rays)), h)
    total = 0
    for p in range(5):
        key = torch.cat([a[p][0], b[p][0]])
        bits = torch.cat([a[p][1], b[p][1]], 1)
        assert torch.equal(key, whole[p][0]), p                  # (the halves' keys are disjoint and ascending)
        assert torch.equal(bits, whole[p][1]), (p, int((bits != whole[p][1]).any(0).sum()))
        total += key.numel()
    assert total > 4096
    assert any(a[p][0].numel() % 64 for p in range(5))           # the second half's pairs sit in other lanes than in the one call


def test_second_batch_of_a_workgroup():
    """GPU only: a quarter of the bench frame's pairs."""
    frame = dict(H=256, W=256, seed=0, cam_dist=1.8)
    net, ctx, rays = world(frame, 128)
    try:
        n = rays[0].shape[0]
        st, v = geometry(net, ctx, rays, 128, max_active=n * 128 // 4)
        counts = check_lists(net, ctx, rays, st, v, 128)
        print('list counts', counts)
        assert max(counts) > GRID_CAP, counts
    finally:
        _CACHE.pop((DEV, 128, tuple(sorted(frame.items()))), None)
