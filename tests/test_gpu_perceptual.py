"""GPU: the perceptual (cfg.use_lpips) image term's kernels (csrc/k_perceptual.hip) through the C ABI of include/invr_perceptual.h.

The gradient of this loss is piecewise constant in ~1.7 M ReLU / sign / pool decisions, and an independent evaluation flips a few of
them (tests/perceptual_reference.py), so every check here is LAYER-LOCAL: each stored convolution output against the float64
convolution of the kernel's OWN stored input to that layer, element by element,

    |kernel - exact|  <=  (c + 4) 2^-24 A  +  c 2^-126          c = 9 C_in + 1 forward, 9 C_out backward; A = the same sum of absolutes

and every discrete rule (ReLU mask, sign, first-maximum pool routing, patch assembly, the sign terms' coefficients) exactly, as a
function of the kernel's own stored values.  End to end the loss is held to 8 noise of the float64 loss of the original inputs and
g_rgb to 8 noise + (c + 4) 2^-24 A of the float64 backward with the kernel's decisions; noise = max(deviation of the checker's fp32
mode, move of `exact` under four ulp-sized input perturbations).  Nothing is fitted to the kernel.  Each case prints
K = max error / (noise + 2^-23 A) for the kernel and the fp32 mode (profiles/perceptual_headroom.md keeps them).

Outputs and the workspace are pre-filled: NaN bytes where a kernel must write, a marker where it must not.
tests/test_hostsim_perceptual_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import perceptual_reference as R          # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
MARK = -0x365A5A5B                                   # int32 bit pattern of a float no kernel may produce here
G_LOSS = 0.7

SHAPES = ((2, 2), (3, 3), (8, 8), (9, 7), (16, 16), (17, 15), (24, 40), (33, 16))
MASKS = ('full', 'p80', 'one')
SIGMAS = (0.05, 0.002)
SMALL = ['%dx%d-%s-%g' % (h, w, m, s) for h, w in SHAPES for m in MASKS for s in SIGMAS]
LARGE = ['56x56-p80-0.05', '64x64-p80-0.002']          # the production sizes
CASES = SMALL + LARGE


def parse(case):
    hw, m, s = case.split('-', 2)
    h, w = hw.split('x')
    return int(h), int(w), m, float(s)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """-> H, W, mask (H*W uint8), rgb (n, 3) in [0, 1], gt = clamp(rgb + N(0, sigma^2)): all fp32 CPU tensors, seeded by the case."""
    H, W, m, sigma = parse(case)
    g = torch.Generator().manual_seed(H * 10007 + W * 101 + MASKS.index(m) * 7 + int(sigma * 1e4))
    if m == 'full':
        mask = torch.ones(H * W, dtype=torch.uint8)
    elif m == 'p80':
        mask = (torch.rand(H * W, generator=g) < 0.8).to(torch.uint8)
    else:
        mask = torch.zeros(H * W, dtype=torch.uint8)
        mask[int(torch.randint(0, H * W, (1,), generator=g))] = 1
    n = int(mask.sum())
    rgb = torch.rand(n, 3, generator=g)
    gt = (rgb + torch.randn(n, 3, generator=g) * sigma).clamp(0.0, 1.0)
    return H, W, mask, rgb, gt


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    """uint8 tensor of nbytes on DEV at a 256-byte-aligned address, every byte `fill`."""
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


_PACKED = {}


def weights():
    return R.make_weights(0)


def packed():
    """The packed weight image of the test weights on DEV (built once per device / library)."""
    key = (DEV, id(_abi.lib()))
    if key not in _PACKED:
        ws, bs = weights()
        _PACKED[key] = _abi.perceptual_pack([t.to(DEV) for t in ws], [t.to(DEV) for t in bs])
        sync()
    return _PACKED[key]


def run_raw(H, W, mask, rgb, gt, fill=0xFF, g_loss=G_LOSS, backward=True):
    """One invr_perceptual_fwd (+ _bwd) over a fresh workspace of `fill` bytes -> dict of CPU tensors: every workspace view, out8,
    g_rgb (n, 3).  The guard rows behind out8 and g_rgb are asserted untouched."""
    L = _abi.lib()
    n = rgb.shape[0]
    nbytes = L.invr_perceptual_workspace_bytes(H, W)
    assert nbytes > 0
    ws = aligned_bytes(nbytes, fill)
    out8 = torch.full((16,), float('nan'))
    out8[8:] = torch.full((8,), MARK, dtype=torch.int32).view(torch.float32)
    g_rgb = torch.full((n + 4, 3), MARK, dtype=torch.int32).view(torch.float32).clone()
    g_rgb[:n] = float('nan')
    out8, g_rgb = out8.to(DEV), g_rgb.to(DEV)
    mask_d, rgb_d, gt_d = mask.to(DEV), rgb.contiguous().to(DEV), gt.contiguous().to(DEV)
    gl = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    pk = packed()
    _abi.check(L.invr_perceptual_fwd(_abi.ptr(pk), _abi.ptr(rgb_d), _abi.ptr(gt_d), _abi.ptr(mask_d, torch.uint8), n, H, W,
                                     _abi.ptr(ws, torch.uint8), nbytes, _abi.ptr(out8), _abi.stream_ptr()))
    if backward:
        _abi.check(L.invr_perceptual_bwd(_abi.ptr(pk), _abi.ptr(mask_d, torch.uint8), n, H, W, _abi.ptr(ws, torch.uint8), nbytes, _abi.ptr(gl),
                                         _abi.ptr(g_rgb), _abi.stream_ptr()))
    sync()
    v = _abi.perceptual_views(ws, H, W)
    lay = v.pop('layout')
    r = {k: t.cpu().clone() for k, t in v.items()}
    r['n_part1'], r['n_part2'] = lay.n_part1, lay.n_part2
    out8, g_rgb = out8.cpu(), g_rgb.cpu()
    assert (out8[8:].view(torch.int32) == MARK).all() and (g_rgb[n:].contiguous().view(torch.int32) == MARK).all(), 'written past an output'
    r['out8'], r['g_rgb'] = out8[:8], g_rgb[:n]
    return r


@functools.lru_cache(maxsize=None)
def run(case, dev):
    return run_raw(*inputs(case))


def bits(t):
    return t.contiguous().view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def within(kernel, exact, A, c):
    return bool(((kernel.double() - exact).abs() <= R.bound(c, A)).all())


# ---- layer-local forward ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_forward_layers(case):
    H, W, mask, rgb, gt = inputs(case)
    r = run(case, DEV)
    ws, bs = weights()
    # the assembled images and the ranks: zeros; img[mask] = rgb
    assert same_bits(r['img'][0], R.assemble(rgb, mask, H, W)) and same_bits(r['img'][1], R.assemble(gt, mask, H, W))
    rank = torch.full((H * W,), -1, dtype=torch.int32)
    rank[mask.bool()] = torch.arange(rgb.shape[0], dtype=torch.int32)
    assert torch.equal(r['rank'].reshape(-1), rank)
    # each of the 4 + 4 convolution outputs against the float64 convolution of the kernel's own stored input
    for l, (src, dst) in enumerate((('img', 'a11'), ('a11', 'a12'), ('pool', 'a21'), ('a21', 'a22'))):
        exact, A, c = R.conv_fwd(r[src], ws[l], bs[l])
        s = r[dst].double()
        bd = R.bound(c, A)
        assert torch.isfinite(r[dst]).all() and (s >= 0).all(), dst
        ok = torch.where(s > 0, (s - exact).abs() <= bd, exact <= bd)          # exactly max(pre, 0) of a value within the bound
        assert ok.all(), (dst, float(((s - exact.clamp(min=0)).abs() / bd).max()))
    assert same_bits(r['pool'], R.pool(r['a12']))


# ---- layer-local backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_backward_layers(case):
    H, W, mask, rgb, gt = inputs(case)
    r = run(case, DEV)
    if rgb.shape[0] == 0:
        return
    ws, _ = weights()
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    zero = torch.zeros((), dtype=torch.float32)
    n1, n2, ni = r['a12'][0].numel(), r['a22'][0].numel(), r['img'][0].numel()
    # the sign terms, with their coefficients exactly g_loss / (2 numel) in fp32, and the masks implied by the stored activations
    k2 = f32(G_LOSS) / (f32(2.0) * f32(float(n2)))
    assert same_bits(r['g22'], k2 * torch.sign(r['a22'][0] - r['a22'][1]))
    assert same_bits(r['gm22'], torch.where(r['a22'][0] > 0, r['g22'], zero))
    exact, A, c = R.conv_bwd(r['gm22'][None], ws[3])
    assert within(r['g21'], exact[0], A[0], c), 'g21'
    assert same_bits(r['gm21'], torch.where(r['a21'][0] > 0, r['g21'], zero))
    exact, A, c = R.conv_bwd(r['gm21'][None], ws[2])
    assert within(r['gpool'], exact[0], A[0], c), 'gpool'
    # the pool routes to the FIRST maximum of the stored window; + the relu1_2 sign term: one fp32 addition
    k1 = f32(G_LOSS) / (f32(2.0) * f32(float(n1)))
    first = R.pool_first(r['a12'][0])
    assert same_bits(r['g12'], R.pool_route(r['gpool'], first, H, W) + k1 * torch.sign(r['a12'][0] - r['a12'][1]))
    assert same_bits(r['gm12'], torch.where(r['a12'][0] > 0, r['g12'], zero))
    exact, A, c = R.conv_bwd(r['gm12'][None], ws[1])
    assert within(r['g11'], exact[0], A[0], c), 'g11'
    assert same_bits(r['gm11'], torch.where(r['a11'][0] > 0, r['g11'], zero))
    # the image: conv1_1's data gradient + the image's L1 sign term + its MSE term (two more summands)
    exact, A, c = R.conv_bwd(r['gm11'][None], ws[0])
    d = r['img'][0] - r['img'][1]
    kl, km = (f32(G_LOSS) / f32(float(ni))).double(), (f32(G_LOSS) * f32(2.0) / f32(float(ni))).double()
    t1, t2 = kl * torch.sign(d).double(), km * d.double()
    assert within(r['gimg'], exact[0] + t1 + t2, A[0] + t1.abs() + t2.abs(), c + 2), 'gimg'
    # gradients of masked-out pixels are dropped, the others go to their ray
    assert same_bits(r['g_rgb'], r['gimg'].reshape(3, -1)[:, mask.bool()].t().contiguous())


# ---- the four means and out8 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES)
def test_means_and_out8(case):
    r = run(case, DEV)
    n1, n2 = r['n_part1'], r['n_part2']
    d1, d2, di = (r['a12'][0] - r['a12'][1]), (r['a22'][0] - r['a22'][1]), (r['img'][0] - r['img'][1])          # fp32 differences, as the kernel's
    sums = (d1.abs().double().sum(), d2.abs().double().sum(), di.abs().double().sum(), (di * di).double().sum())
    got = (r['partial'][:n1].sum(), r['partial'][n1:n1 + n2].sum(), r['partial'][n1 + n2], r['partial'][n1 + n2 + 1])
    for k in range(4):          # float64 accumulation: 2^-53 per summand, far inside the fp32 form of the bound
        assert abs(float(got[k] - sums[k])) <= float(R.bound(1, sums[k])), (k, float(got[k]), float(sums[k]))
    means = [sums[0] / d1.numel(), sums[1] / d2.numel(), sums[2] / di.numel(), sums[3] / di.numel()]
    for k in range(4):          # each mean: one rounding to fp32
        assert abs(float(r['out8'][1 + k].double() - means[k])) <= float(R.bound(1, means[k])), (k, float(r['out8'][1 + k]), float(means[k]))
    lp = (means[0] + means[1]) / 2.0 + means[2] + means[3]
    assert abs(float(r['out8'][0].double() - lp)) <= float(R.bound(1, lp))
    assert (bits(r['out8'][5:]) == 0).all()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def perturbed(t, g):
    return t.double() * (1.0 + (torch.randint(0, 2, t.shape, generator=g).double() * 2.0 - 1.0) * 2.0 ** -23)


@pytest.mark.parametrize('case', CASES)
def test_end_to_end(case):
    H, W, mask, rgb, gt = inputs(case)
    r = run(case, DEV)
    ws, bs = weights()
    img = lambda v: R.assemble(v, mask, H, W)
    dec = R.Decisions.of(r)                                                            # the kernel's own decisions
    f64 = R.forward(ws, bs, img(rgb.double()), img(gt.double()))
    f32m = R.forward(ws, bs, img(rgb), img(gt), torch.float32)
    b64 = R.backward(ws, img(rgb.double()), img(gt.double()), dec, G_LOSS)
    b32 = R.backward(ws, img(rgb), img(gt), dec, G_LOSS, torch.float32)
    noise_l = (f32m['loss'].double() - f64['loss']).abs()
    noise_g = (b32['gimg'].double() - b64['gimg']).abs()
    g = torch.Generator().manual_seed(77)
    for _ in range(4):
        pr, pg = perturbed(rgb, g), perturbed(gt, g)
        noise_l = torch.maximum(noise_l, (R.forward(ws, bs, img(pr), img(pg))['loss'] - f64['loss']).abs())
        noise_g = torch.maximum(noise_g, (R.backward(ws, img(pr), img(pg), dec, G_LOSS)['gimg'] - b64['gimg']).abs())
    err_l = (r['out8'][0].double() - f64['loss']).abs()
    sel = lambda t: t.reshape(3, -1)[:, mask.bool()].t()
    err_g = (r['g_rgb'].double() - sel(b64['gimg'])).abs()
    ng, Ag = sel(noise_g), sel(b64['A'])
    if rgb.shape[0]:
        K = float((err_g / (ng + 2.0 ** -23 * Ag + 1e-300)).max())
        K32 = float((sel((b32['gimg'].double() - b64['gimg']).abs()) / (ng + 2.0 ** -23 * Ag + 1e-300)).max())
        print('perceptual %-18s loss K %.3f (fp32 mode %.3f)   g_rgb K %.3f (fp32 mode %.3f)'
              % (case, float(err_l / (noise_l + 2.0 ** -23 * f64['A'])), float((f32m['loss'].double() - f64['loss']).abs() / (noise_l + 2.0 ** -23 * f64['A'])),
                 K, K32))
    assert float(err_l) <= 8.0 * float(noise_l), (float(err_l), float(noise_l))
    assert (err_g <= 8.0 * ng + R.bound(b64['c'], Ag)).all()


# ---- exactness ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ('8x8-full-0.05', '17x15-p80-0.05', '33x16-p80-0.002'))
def test_identical_images_give_exact_zero(case):
    H, W, mask, rgb, _ = inputs(case)
    r = run_raw(H, W, mask, rgb, rgb.clone())
    assert (bits(r['out8']) == 0).all()                              # +0.0, every entry
    assert (bits(r['g_rgb']) & 0x7fffffff == 0).all()                # exactly 0.0
    for k in ('a11', 'a12', 'pool', 'a21', 'a22'):
        assert same_bits(r[k][0], r[k][1]), k


def dilate(m):
    return torch.nn.functional.max_pool2d(m[None, None].float(), 3, 1, 1)[0, 0] > 0


@pytest.mark.parametrize('case', ('17x15-full-0.05', '24x40-p80-0.05', '33x16-full-0.002'))
def test_one_pixel_difference_stays_inside_its_receptive_field(case):
    H, W, mask, rgb, _ = inputs(case)
    gt = rgb.clone()
    row = rgb.shape[0] // 2
    gt[row] = (gt[row] + 0.25) % 1.0
    r = run_raw(H, W, mask, rgb, gt)
    hit = (r['rank'] == row)
    assert int(hit.sum()) == 1
    f11 = dilate(hit)
    f12 = dilate(f11)
    fp = torch.nn.functional.max_pool2d(f12[None, None].float(), 2, 2)[0, 0] > 0
    f21 = dilate(fp)
    f22 = dilate(f21)
    for k, f in (('img', hit), ('a11', f11), ('a12', f12), ('pool', fp), ('a21', f21), ('a22', f22)):
        outside = ~f
        assert (bits(r[k][0])[:, outside] == bits(r[k][1])[:, outside]).all(), k
        assert (bits(r[k][0])[:, f] != bits(r[k][1])[:, f]).any() or k != 'img', k
    assert (bits(r['g22'])[:, ~f22] & 0x7fffffff == 0).all() and (bits(r['g12'] - R.pool_route(r['gpool'], R.pool_first(r['a12'][0]), H, W))[:, ~f12]
                                                                  & 0x7fffffff == 0).all()


@pytest.mark.parametrize('hw', ((2, 2), (9, 7), (17, 15)))
def test_no_rays(hw):
    H, W = hw
    r = run_raw(H, W, torch.zeros(H * W, dtype=torch.uint8), torch.zeros(0, 3), torch.zeros(0, 3))
    assert (bits(r['out8']) == 0).all()
    assert r['g_rgb'].numel() == 0                                   # (run_raw asserted the rows behind it untouched)
    assert (r['rank'] == -1).all() and (bits(r['img']) == 0).all()


@pytest.mark.parametrize('case', ('9x7-p80-0.05', '17x15-p80-0.002', '24x40-full-0.05'))
def test_two_runs_over_dirty_workspaces_are_bit_identical(case):
    a = run(case, DEV)
    b = run_raw(*inputs(case), fill=0x5A)
    for k in a:
        if torch.is_tensor(a[k]):
            assert same_bits(a[k], b[k]), k


def test_mask_bits_beyond_n_rays_are_ignored():
    """More set bytes than rays: the surplus pixels are treated as unset (nothing is read past rgb's end)."""
    H, W, mask, rgb, gt = inputs('9x7-p80-0.05')
    n = rgb.shape[0] - 5
    r = run_raw(H, W, mask, rgb[:n].clone(), gt[:n].clone())
    rank = r['rank'].reshape(-1)
    assert int((rank >= 0).sum()) == n and int(rank.max()) == n - 1
    assert torch.isfinite(r['g_rgb']).all()


def test_argument_checks_launch_nothing():
    L = _abi.lib()
    pk = packed()
    ws = aligned_bytes(L.invr_perceptual_workspace_bytes(8, 8), 0xFF)
    z = torch.zeros(64, 3, device=DEV)
    m = torch.ones(64, dtype=torch.uint8, device=DEV)
    o = torch.zeros(8, device=DEV)
    args = lambda H, W, n, nbytes: (_abi.ptr(pk), _abi.ptr(z), _abi.ptr(z), _abi.ptr(m, torch.uint8), n, H, W, _abi.ptr(ws, torch.uint8), nbytes,
                                    _abi.ptr(o), _abi.stream_ptr())
    assert L.invr_perceptual_fwd(*args(1, 8, 8, ws.numel())) != 0 and b'H, W must be in' in L.invr_last_error()
    assert L.invr_perceptual_fwd(*args(8, 8, 65, ws.numel())) != 0 and b'n_rays' in L.invr_last_error()
    assert L.invr_perceptual_fwd(*args(8, 8, 64, ws.numel() - 1)) != 0 and b'workspace too small' in L.invr_last_error()
    sync()
    assert (ws == 0xFF).all()
