"""GPU: three training-side entry points that had no stage test of their own, against float64.

invr_distortion_fwd vs the oracle's distortion_loss in float64 at ragged shapes (S below / at / above one wave, one ray per
workgroup tail), weights ~60 % exact zeros, jittered ascending z:
    |kernel - exact| <= 8 noise + 2 S 2^-24 value
noise = the larger of the fp32 oracle's deviation and the largest move of the float64 value under 4 ulp-sized perturbations of z
(tests/conditioning.py's convention: |m_i - m_j| of neighbouring samples cancels).  All summands are non-negative, so the value is its
own absolute sum; 2 S bounds the depth of a sum taken row by row and then over the rows (S + S/64 + 6 additions, 5 roundings per term).

invr_distortion_bwd vs float64 autograd of the same function with respect to the weights, on the same inputs: the same form of bound
with A = 2 |g| sum_j |w_j| |m_i - m_j| (test_distortion_bwd_vs_float64).

invr_train_loss_fwd / _bwd vs the closed form of include/invr.h in float64.  The forward sums in double, so what is left are the
fp32 roundings of a term (d = rgb - gt, d * d: (1 + e)^3), the final casts and one division each:
    img_loss, reg_dist, offset_loss, pair_loss   8 2^-24 relative
    loss                                          8 2^-24 sum |terms|
    psnr                                          4.343 * 16 2^-24 + 4 2^-24 |psnr|     (d psnr = 4.343 d img / img; logf, the division)
    err                                           4 2^-24 sum_c |d|
    backward elements                             8 2^-24 relative; g_terms slots other than the two used exactly 0

tests/test_hostsim_encoder_bwd_cpu.py runs the same bodies on the CPU wave machine."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nvr_oracle as O          # noqa: E402  (checker only)
from invr import _abi                       # noqa: E402

DEV = 'cuda:0'
U = 2.0 ** -24


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


@pytest.mark.parametrize('R,S', [(1, 1), (7, 5), (33, 64), (20, 65), (9, 128), (5, 200), (4097, 64)])
def test_distortion_fwd_vs_float64(R, S):
    g = torch.Generator().manual_seed(100 * R + S)
    w = torch.rand(R, S, generator=g) * (torch.rand(R, S, generator=g) > 0.6) * (2.0 / S)
    if R > 2:
        w[1] = 0.0                                                          # a ray that hit nothing
    z = 2.0 + 2.0 * (torch.arange(S)[None] + torch.rand(R, S, generator=g) * 0.9) / S        # ascending, jittered
    assert (z[:, 1:] > z[:, :-1]).all()
    out = torch.full((R,), float('nan'), device=DEV)
    wd, zd = w.to(DEV).contiguous(), z.to(DEV).contiguous()
    _abi.check(_abi.lib().invr_distortion_fwd(_abi.ptr(wd), _abi.ptr(zd), R, S, _abi.ptr(out), _abi.stream_ptr()))
    sync()
    out = out.cpu()
    exact = O.distortion_loss(w.double(), z.double())
    o32 = O.distortion_loss(w, z)
    noise = (o32.double() - exact).abs()
    for _ in range(4):
        s = torch.randint(0, 2, z.shape, generator=g).double() * 2.0 - 1.0
        noise = torch.maximum(noise, (O.distortion_loss(w.double(), z.double() * (1.0 + s * 2.0 ** -23)) - exact).abs())
    allow = 8.0 * noise + 2.0 * S * U * exact
    err = (out.double() - exact).abs()
    den = noise + 2.0 * U * exact
    print('DIST R %d S %d  K_kernel %.3g K_oracle32 %.3g' % (R, S, float((err / den.clamp(min=1e-300)).max()),
                                                             float(((o32.double() - exact).abs() / den.clamp(min=1e-300)).max())))
    assert not torch.isnan(out).any()
    assert (err <= allow).all(), float((err - allow).max())
    assert (out[exact == 0] == 0).all()


def _distortion_inputs(R, S):
    """The inputs of test_distortion_fwd_vs_float64 (same seed, same draws in the same order) -> (w, z, generator)."""
    g = torch.Generator().manual_seed(100 * R + S)
    w = torch.rand(R, S, generator=g) * (torch.rand(R, S, generator=g) > 0.6) * (2.0 / S)
    if R > 2:
        w[1] = 0.0
    z = 2.0 + 2.0 * (torch.arange(S)[None] + torch.rand(R, S, generator=g) * 0.9) / S
    return w, z, g


@pytest.mark.parametrize('R,S', [(1, 1), (7, 5), (33, 64), (20, 65), (9, 128), (5, 200), (4097, 64)])
def test_distortion_bwd_vs_float64(R, S):
    """invr_distortion_bwd vs float64 autograd of the oracle's distortion_loss with respect to the weights, on the forward test's
    inputs and a seeded non-zero g_dist, every element:
        |kernel - exact| <= 8 noise + 2 S 2^-24 A,        A = 2 |g| sum_j |w_j| |m_i - m_j|
    noise as in the forward test (the fp32 autograd's deviation; 4 ulp-sized perturbations of z).  The rows of an all-zero ray are
    exactly 0."""
    w, z, g = _distortion_inputs(R, S)
    gd = torch.randn(R, generator=g)
    gd = torch.where(gd.abs() < 0.05, torch.full_like(gd, 0.5), gd)           # non-zero
    out = torch.full((R, S), float('nan'), device=DEV)
    wd, zd, gdd = w.to(DEV).contiguous(), z.to(DEV).contiguous(), gd.to(DEV).contiguous()
    _abi.check(_abi.lib().invr_distortion_bwd(_abi.ptr(wd), _abi.ptr(zd), _abi.ptr(gdd), R, S, _abi.ptr(out), _abi.stream_ptr()))
    sync()
    out = out.cpu()

    def grad(wt, zt, dtype):
        wt = wt.to(dtype).clone().requires_grad_()
        O.distortion_loss(wt, zt.to(dtype)).backward(gd.to(dtype))
        return wt.grad
    exact = grad(w, z, torch.float64)
    o32 = grad(w, z, torch.float32)
    noise = (o32.double() - exact).abs()
    for _ in range(4):
        s = torch.randint(0, 2, z.shape, generator=g).double() * 2.0 - 1.0
        noise = torch.maximum(noise, (grad(w, z.double() * (1.0 + s * 2.0 ** -23), torch.float64) - exact).abs())
    nz = torch.cat([z[:, 1:], z[:, -1:]], -1).double()
    mid = (z.double() + nz) / 2
    A = 2.0 * gd.double().abs()[:, None] * (w.double().abs()[:, None, :] * (mid[:, :, None] - mid[:, None, :]).abs()).sum(-1)
    assert (A >= exact.abs() * (1 - 1e-12)).all()
    allow = 8.0 * noise + 2.0 * S * U * A
    err = (out.double() - exact).abs()
    den = noise + 2.0 * U * A
    print('DISTB R %d S %d  K_kernel %.3g K_oracle32 %.3g' % (R, S, float((err / den.clamp(min=1e-300)).max()),
                                                              float(((o32.double() - exact).abs() / den.clamp(min=1e-300)).max())))
    assert not torch.isnan(out).any()
    assert (err <= allow).all(), float((err - allow).max())
    assert (out[A == 0] == 0).all()
    if R > 2:
        assert not w[1].any() and (out[1] == 0).all()                           # the ray that hit nothing


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1023, 1025, 4096, 65536 + 3])
def test_train_loss_fwd_bwd_vs_closed_form(n):
    L = _abi.lib()
    g = torch.Generator().manual_seed(n)
    w_pair, w_dist, w_off = _f32(0.01), _f32(0.1), _f32(0.02)
    for scale in (1e-4, 0.3):                                               # psnr 80 dB / a bad frame
        gt = torch.rand(n, 3, generator=g)
        rgb = (gt + scale * torch.randn(n, 3, generator=g)).float()
        dist = torch.rand(n, generator=g) * 1e-2
        for has_dist in (True, False):
            for use_pair in (0, 1):
                for rows in (0.0, 12345.0):
                    terms = torch.tensor([37.25 * (rows > 0) + 0.3, rows, 4.5, rows and 321.0, 9.0, 9.0, 9.0, 9.0])
                    out = torch.full((8,), float('nan'), device=DEV)
                    err = torch.full((n,), float('nan'), device=DEV)
                    rd_, gd_, dd_, td_ = rgb.to(DEV), gt.to(DEV), dist.to(DEV), terms.to(DEV)
                    _abi.check(L.invr_train_loss_fwd(_abi.ptr(rd_), _abi.ptr(gd_), _abi.ptr(dd_ if has_dist else None), _abi.ptr(td_), n,
                                                     w_pair, w_dist, w_off, use_pair, _abi.ptr(out), _abi.ptr(err), _abi.stream_ptr()))
                    gl = torch.tensor([0.7], device=DEV)
                    g_rgb = torch.full((n, 3), float('nan'), device=DEV)
                    g_dist = torch.full((n,), float('nan'), device=DEV) if has_dist else None
                    g_terms = torch.full((8,), float('nan'), device=DEV)
                    _abi.check(L.invr_train_loss_bwd(_abi.ptr(rd_), _abi.ptr(gd_), _abi.ptr(td_), n, w_pair, w_dist, w_off, use_pair,
                                                     _abi.ptr(gl), _abi.ptr(g_rgb), _abi.ptr(g_dist), _abi.ptr(g_terms), _abi.stream_ptr()))
                    sync()
                    out, err, g_rgb, g_terms = out.cpu().double(), err.cpu().double(), g_rgb.cpu().double(), g_terms.cpu()
                    # the closed form (include/invr.h) in float64
                    d = rgb.double() - gt.double()
                    img = (d * d).mean()
                    rdist = dist.double().mean() if has_dist else torch.tensor(0.0, dtype=torch.float64)
                    t = terms.double()
                    off = t[0] / max(float(t[1]), 1.0)
                    pair = t[2] / max(float(t[3]), 1.0) if use_pair else torch.tensor(0.0, dtype=torch.float64)
                    parts = [w_pair * pair, w_dist * rdist, w_off * off, img]
                    loss, psnr = sum(parts), -10.0 * torch.log10(img)
                    what = (n, scale, has_dist, use_pair, rows)
                    for name, got, want in (('img', out[1], img), ('reg_dist', out[3], rdist), ('offset', out[4], off), ('pair', out[5], pair)):
                        assert abs(got - want) <= 8 * U * abs(want), (name, what, float(got), float(want))
                    assert abs(out[0] - loss) <= 8 * U * sum(abs(p) for p in parts), (what, float(out[0]), float(loss))
                    assert abs(out[2] - psnr) <= 4.343 * 16 * U + 4 * U * abs(psnr), (what, float(out[2]), float(psnr))
                    assert out[6] == 0 and out[7] == 0
                    e = d.abs().sum(1)
                    assert ((err - e).abs() <= 4 * U * e).all(), what
                    # backward: d loss / d rgb = 2 d / (3 n), d loss / d dist = w_dist / n, the two sums' 1 / max(rows, 1)
                    k = float(gl.cpu().double()[0])
                    want = k * 2.0 * d / (3 * n)
                    assert ((g_rgb - want).abs() <= 8 * U * want.abs()).all(), what
                    if has_dist:
                        wd = k * w_dist / n
                        assert ((g_dist.cpu().double() - wd).abs() <= 8 * U * abs(wd)).all(), what
                    gt_off = k * w_off / max(float(t[1]), 1.0)
                    gt_pair = k * w_pair / max(float(t[3]), 1.0) if use_pair else 0.0
                    assert abs(float(g_terms[0]) - gt_off) <= 8 * U * abs(gt_off), what
                    assert abs(float(g_terms[2]) - gt_pair) <= 8 * U * abs(gt_pair), what
                    assert all(float(g_terms[i]) == 0.0 for i in (1, 3, 4, 5, 6, 7)), (what, g_terms.tolist())
