"""GPU: the evaluator's LPIPS kernels (csrc/k_lpips.hip) through the C ABI of include/invr_lpips.h.

Every check of the network is LAYER-LOCAL (keep = 1 stores every array): each of the 13 stored convolution outputs against the float64
convolution of the kernel's OWN stored input to that layer, every element judged,

    |kernel - exact|  <=  (c + 4) 2^-24 A  +  c 2^-126          c = 9 C_in + 1; A = the same sum of absolutes

(the kernel accumulates bias + 9 C_in exact fp32 products in fp32, one chain per element; conv1_1's padded fourth channel adds exact
zeros), the scaled input, the ReLU and every pooled map exactly as functions of the kernel's own values.

Each layer_l is held to the float64 distance of the kernel's own stored tap within (4 C + 2 pixels + 32) 2^-53 A_l, A_l the same mean
with (|n0| + |n1|)^2 in the place of (n0 - n1)^2: the bound on two float64 evaluations that differ in the order of their sums, derived
in tests/lpips_reference.py:distance_rel (rounding counts of S, sqrt, + eps, the quotient, the difference — whose error is relative
to |n0| + |n1|, not to itself — the square, the product with lin and the three sums).  out8[0] is the stated left-to-right sum of
the five, bit for bit.

End to end |lpips - float64 value of the original images| <= 8 noise, noise = max(deviation of the checker's fp32 mode from float64,
move of the float64 value under four ulp-sized input perturbations): the rule of tests/test_gpu_perceptual.py.  Nothing is fitted to
the kernel.  Each case prints K = error / noise for the kernel and for the fp32 mode (profiles/eval_lpips.md keeps them).

The workspace is pre-filled with NaN bytes; the rows behind out8 carry a marker that must survive.
tests/test_hostsim_lpips_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lpips_reference as R               # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
MARK = -0x365A5A5B365A5A5B                           # int64 pattern no kernel writes

SHAPES = ((16, 16), (17, 19), (16, 67), (37, 53), (48, 64))
SIGMAS = (0.05, 0.002)
# 48 x 130: the smallest frame on which block 5 (a 3 x 8 map: strips of 8 x 2) has more than one wave at work, as blocks 1..4 have from 37 x 53 on
CASES = ['%dx%d-rand-%g' % (h, w, s) for h, w in SHAPES for s in SIGMAS] + ['37x53-mask-0.05', '48x130-rand-0.05']
PROPS = ['16x16-rand-0.05', '17x19-rand-0.002', '37x53-mask-0.05']


def parse(case):
    hw, kind, s = case.split('-', 2)
    h, w = hw.split('x')
    return int(h), int(w), kind, float(s)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> pred (H, W, 3) uniform in [0, 1], gt = clamp(pred + N(0, sigma^2)); kind 'mask': both exactly zero outside a rectangle."""
    H, W, kind, sigma = parse(case)
    g = torch.Generator().manual_seed(H * 10007 + W * 101 + (kind == 'mask') * 7 + int(sigma * 1e4))
    pred = torch.rand(H, W, 3, generator=g)
    gt = (pred + torch.randn(H, W, 3, generator=g) * sigma).clamp(0.0, 1.0)
    if kind == 'mask':
        m = torch.zeros(H, W, 1)
        m[H // 4:3 * H // 4, W // 5:4 * W // 5] = 1.0
        pred, gt = pred * m, gt * m
    return pred.contiguous(), gt.contiguous()


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


@functools.lru_cache(maxsize=None)
def weights():
    return R.make_weights(0)


_PACKED = {}


def packed():
    key = (DEV, id(_abi.lib()))
    if key not in _PACKED:
        cw, cb, lw = weights()
        to = lambda ts: [t.to(DEV) for t in ts]
        _PACKED[key] = _abi.lpips_pack(to(cw), to(cb), to(lw), torch.tensor(R.SHIFT, device=DEV), torch.tensor(R.SCALE, device=DEV))
        sync()
    return _PACKED[key]


def run_raw(pred, gt, keep=1, fill=0xFF, ws=None):
    """One invr_lpips_fwd over a workspace of `fill` bytes (or the caller's `ws`) -> dict of CPU tensors: out8 and, with keep = 1, every
    workspace view.  The rows behind out8 are asserted untouched."""
    L = _abi.lib()
    H, W = pred.shape[:2]
    nbytes = L.invr_lpips_workspace_bytes(H, W, keep)
    assert nbytes > 0
    if ws is None:
        ws = aligned_bytes(nbytes, fill)
    out = torch.full((16,), float('nan'), dtype=torch.float64)
    out[8:] = torch.full((8,), MARK, dtype=torch.int64).view(torch.float64)
    out, pred_d, gt_d = out.to(DEV), pred.to(DEV), gt.to(DEV)          # (held until the call has been joined)
    _abi.check(L.invr_lpips_fwd(_abi.ptr(packed()), _abi.ptr(pred_d), _abi.ptr(gt_d), H, W, keep, _abi.ptr(ws, torch.uint8),
                                C.c_size_t(ws.numel()), _abi.ptr(out, torch.float64), _abi.stream_ptr()))
    sync()
    out = out.cpu()
    assert (out[8:].view(torch.int64) == MARK).all(), 'written past out8'
    r = {'out8': out[:8].clone()}
    if keep:
        v = _abi.lpips_views(ws, H, W)
        r['scaled'] = v['scaled'].cpu().clone()
        for k in ('act', 'pool', 'partial'):
            r[k] = [t.cpu().clone() for t in v[k]]
    return r


@functools.lru_cache(maxsize=None)
def run(case, dev):
    return run_raw(*inputs(case))


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def all_same(a, b):
    for k in a:
        for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
            assert same_bits(x, y), k


# ---- layer-local ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_forward_layers(case):
    pred, gt = inputs(case)
    r = run(case, DEV)
    cw, cb, _ = weights()
    # the scaling layer: one fp32 subtraction and one fp32 division; a zero pixel becomes -shift / scale
    assert same_bits(r['scaled'][0], R.scale_layer(pred, torch.float32)) and same_bits(r['scaled'][1], R.scale_layer(gt, torch.float32))
    for l in range(13):
        first = l > 0 and R.BLOCK[l] != R.BLOCK[l - 1]
        src = r['scaled'] if l == 0 else (r['pool'][R.BLOCK[l] - 1] if first else r['act'][l - 1])
        if first:
            assert same_bits(src, R.pool(r['act'][l - 1])), ('pool', l)
        exact, A, c = R.conv_fwd(src, cw[l], cb[l])
        assert c == 9 * R.CIN[l] + 1
        s = r['act'][l].double()
        bd = R.bound(c, A)
        assert s.shape == exact.shape and torch.isfinite(s).all() and (s >= 0).all(), l
        ok = torch.where(s > 0, (s - exact).abs() <= bd, exact <= bd)          # exactly max(pre, 0) of a value within the bound
        assert ok.all(), (l, float(((s - exact.clamp(min=0)).abs() / bd).max()))


@pytest.mark.parametrize('case', CASES)
def test_distances_and_out8(case):
    r = run(case, DEV)
    _, _, lw = weights()
    o = r['out8']
    for t, l in enumerate(R.TAPS):
        f = r['act'][l]
        val, A = R.distance(f, lw[t])
        pixels = f.shape[2] * f.shape[3]
        tol = R.distance_rel(f.shape[1], pixels) * R.U53 * float(A)
        assert abs(float(o[1 + t]) - float(val)) <= tol, (t, float(o[1 + t]), float(val), tol)
        # the fixed slots: one per workgroup of 16 pixels, and their sum is the layer
        assert r['partial'][t].numel() == (pixels + 15) // 16
        assert abs(float(r['partial'][t].sum()) / pixels - float(val)) <= tol
    total = (((float(o[1]) + float(o[2])) + float(o[3])) + float(o[4])) + float(o[5])
    assert same_bits(o[:1], torch.tensor([total], dtype=torch.float64))
    assert (bits(o[6:]) == 0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def perturbed(t, g):
    return t.double() * (1.0 + (torch.randint(0, 2, t.shape, generator=g).double() * 2.0 - 1.0) * 2.0 ** -23)


@functools.lru_cache(maxsize=None)
def oracle(case):
    """-> (float64 lpips of the original images, fp32 mode's value, noise): computed once per case."""
    pred, gt = inputs(case)
    w = weights()
    f64 = float(R.forward(w, pred, gt)['lpips'])
    f32 = float(R.forward(w, pred, gt, torch.float32)['lpips'])
    noise = abs(f32 - f64)
    g = torch.Generator().manual_seed(77)
    for _ in range(4):
        noise = max(noise, abs(float(R.forward(w, perturbed(pred, g), perturbed(gt, g))['lpips']) - f64))
    return f64, f32, noise


@pytest.mark.parametrize('case', CASES)
def test_end_to_end(case):
    r = run(case, DEV)
    f64, f32, noise = oracle(case)
    err = abs(float(r['out8'][0]) - f64)
    print('lpips %-18s value %.9g   K %.3f (fp32 mode %.3f)   noise %.3g' % (case, f64, err / noise, abs(f32 - f64) / noise, noise))
    assert err <= 8.0 * noise, (err, noise)


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', PROPS)
def test_identical_images_give_exact_zero(case):
    pred, _ = inputs(case)
    r = run_raw(pred, pred.clone())
    assert (bits(r['out8']) == 0).all()                              # +0.0 in all six outputs (and the two spare ones)
    for k in ['scaled'] + [('act', l) for l in range(13)] + [('pool', b) for b in range(4)]:
        t = r[k] if isinstance(k, str) else r[k[0]][k[1]]
        assert same_bits(t[0], t[1]), k


@pytest.mark.parametrize('case', PROPS)
def test_swapped_images_give_the_same_bits(case):
    pred, gt = inputs(case)
    assert same_bits(run_raw(gt, pred, keep=0)['out8'], run(case, DEV)['out8'])


@pytest.mark.parametrize('case', PROPS)
def test_two_runs_over_dirty_workspaces_are_bit_identical(case):
    all_same(run(case, DEV), run_raw(*inputs(case), fill=0x5A))


@pytest.mark.parametrize('case', PROPS)
def test_rotating_buffers_give_the_same_bits(case):
    assert same_bits(run_raw(*inputs(case), keep=0)['out8'], run(case, DEV)['out8'])


@pytest.mark.parametrize('case', PROPS)
def test_same_frame_after_a_larger_one_on_the_same_workspace(case):
    pred, gt = inputs(case)
    H, W = pred.shape[:2]
    g = torch.Generator().manual_seed(5)
    big = torch.rand(H + 1, W + 2, 3, generator=g)
    ws = aligned_bytes(_abi.lib().invr_lpips_workspace_bytes(H + 1, W + 2, 0), 0xFF)
    run_raw(big, big.flip(0).contiguous(), keep=0, ws=ws)
    assert same_bits(run_raw(pred, gt, keep=0, ws=ws)['out8'], run(case, DEV)['out8'])


def dilate(m):
    return torch.nn.functional.max_pool2d(m[None, None].float(), 3, 1, 1)[0, 0] > 0


@pytest.mark.parametrize('case', PROPS)
def test_one_pixel_difference_stays_inside_its_receptive_field(case):
    """Both images go through identical arithmetic: outside the changed pixel's receptive field their features are bit-equal."""
    pred, _ = inputs(case)
    H, W = pred.shape[:2]
    gt = pred.clone()
    gt[H // 2, W // 2] = (gt[H // 2, W // 2] + 0.25) % 1.0
    r = run_raw(pred, gt)
    f = torch.zeros(H, W, dtype=torch.bool)
    f[H // 2, W // 2] = True
    fields = [('scaled', r['scaled'], f)]
    for l in range(7):                                               # through relu3_3; beyond it the field covers these maps
        if l > 0 and R.BLOCK[l] != R.BLOCK[l - 1]:
            f = torch.nn.functional.max_pool2d(f[None, None].float(), 2, 2)[0, 0] > 0
            fields.append(('pool%d' % R.BLOCK[l], r['pool'][R.BLOCK[l] - 1], f))
        f = dilate(f)
        fields.append(('act%d' % l, r['act'][l], f))
    for name, t, f in fields:
        assert (bits(t[0])[:, ~f] == bits(t[1])[:, ~f]).all(), name
    assert (bits(r['scaled'][0])[:, fields[0][2]] != bits(r['scaled'][1])[:, fields[0][2]]).any()


def test_argument_checks_launch_nothing():
    L = _abi.lib()
    nb = L.invr_lpips_workspace_bytes(16, 16, 0)
    ws = aligned_bytes(nb, 0xFF)
    z = torch.zeros(16, 16, 3, device=DEV)
    o = torch.zeros(8, dtype=torch.float64, device=DEV)
    args = lambda H, W, nbytes: (_abi.ptr(packed()), _abi.ptr(z), _abi.ptr(z), H, W, 0, _abi.ptr(ws, torch.uint8), C.c_size_t(nbytes),
                                 _abi.ptr(o, torch.float64), _abi.stream_ptr())
    assert L.invr_lpips_fwd(*args(15, 16, nb)) != 0 and b'invr_lpips_fwd: H, W must be in' in L.invr_last_error()
    assert L.invr_lpips_fwd(*args(16, 16, nb - 1)) != 0 and b'workspace too small' in L.invr_last_error()
    sync()
    assert (ws == 0xFF).all()
