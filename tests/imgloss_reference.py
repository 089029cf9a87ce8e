"""Checker only: the SSIM and TV image terms of the training objective (include/invr_imgloss.h; the reference's
lib/utils/loss_utils.py:7-37 and lib/train/trainers/loss/tv_image_loss.py:11-21) in float64, forward and backward, every intermediate
map returned — and, next to every value, a bound on what an fp32 evaluation of the same formula may deviate from it.

The bound is a running error analysis (Higham, Accuracy and Stability of Numerical Algorithms, section 3.3): every quantity is a pair
(v, e) of the exact float64 value and a bound e on |fp32 result - v|.  With u = 2^-24 and inputs a +- ea, b +- eb one fp32 operation gives

    a + b : ea + eb                          + u (|v| + that)        a * b : |a| eb + |b| ea + ea eb + u (|v| + that)
    a / b : (ea + |v| eb) / (|b| - eb)       + u (|v| + that)        sum of n terms: sum e_i + (n - 1) u sum (|t_i| + e_i)  (any order)

so the bound holds for any order of the additions and for fused multiply-adds (fewer roundings).  The Gaussian filter is two passes
of w-term dot products over a window the reference forms as fp32 products g[i] g[j]: (2 w + 3) u G*(|x| + e) + G*e.  The inputs (fp32
images, fp32 taps, an fp32 g_loss) are exact; constants carry u |c|.  A float64 partial sum adds 2^-53 per term: nothing at this scale.
Discrete decisions (TV's relu) whose operand is within its bound of the threshold are reported as undecided: either side is accepted.
Nothing here is fitted to the kernels."""
import math

import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
C1, C2 = 0.01 ** 2, 0.03 ** 2
F64 = torch.float64


class E:
    """value +- bound of its fp32 evaluation (float64 tensors of one shape)"""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64) + torch.zeros_like(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, E) else E.const(x)

    @staticmethod
    def const(c):
        """a constant of the formula, rounded to fp32 by the evaluation"""
        c = torch.as_tensor(c, dtype=F64)
        return E(c, U * c.abs())

    @staticmethod
    def exact(x):
        return E(torch.as_tensor(x).to(F64))

    def _round(self, v, e):
        return E(v, e + U * (v.abs() + e) + TINY)

    def __add__(self, o):
        o = E.of(o)
        return self._round(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = E.of(o)
        return self._round(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = E.of(o)
        return self._round(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)

    def __truediv__(self, o):
        o = E.of(o)
        v = self.v / o.v
        room = o.v.abs() - o.e
        assert bool((room > 0).all()), 'a divisor is not separated from zero'
        return self._round(v, (self.e + v.abs() * o.e) / room)

    def __neg__(self):
        return E(-self.v, self.e)

    def twice(self):
        return E(2.0 * self.v, 2.0 * self.e)

    def sel(self, idx):
        return E(self.v[idx], self.e[idx])

    def holds(self, got, slack=1.0):
        """|got - v| <= slack e, element by element (NaN matches NaN) -> (ok, worst ratio)"""
        got = torch.as_tensor(got).to(F64)
        nan = torch.isnan(self.v)
        d = torch.where(nan, torch.zeros_like(self.v), (got - self.v).abs())
        bound = torch.where(nan, torch.zeros_like(self.v), slack * self.e + TINY)
        ok = bool((torch.isnan(got) == nan).all()) and bool((d <= bound).all())
        ratio = float((d / (bound + TINY)).max()) if d.numel() else 0.0
        return ok, ratio


def gaussian_taps(w, sigma=1.5):
    """loss_utils.py:7-9 as torch evaluates it: doubles rounded to fp32, an fp32 sum, an fp32 division"""
    g = torch.tensor([math.exp(-(x - w // 2) ** 2 / float(2 * sigma ** 2)) for x in range(w)], dtype=torch.float32)
    return g / g.sum()


def assemble(values, mask, H, W):
    """img = zeros(H, W, C); img[mask] = values -> planar (C, H, W), dtype of `values`"""
    values = values.reshape(values.shape[0], values.shape[-1] if values.dim() > 1 else 1)
    img = torch.zeros(H * W, values.shape[1], dtype=values.dtype)
    img[mask.reshape(-1).bool()] = values
    return img.t().reshape(values.shape[1], H, W).contiguous()


def window2d(taps):
    """loss_utils.py:11-15: the fp32 products g[i] g[j], as float64"""
    g = taps.to(torch.float32).unsqueeze(1)
    return g.mm(g.t()).to(F64)


def _conv(x, win):
    w = win.shape[0]
    return torch.nn.functional.conv2d(x[:, None], win[None, None], padding=w // 2)[:, 0]


def gfilter(x, taps):
    """G*x of a (C, H, W) quantity: the zero-padded window of the reference"""
    win = window2d(taps)
    w = taps.numel()
    A = _conv(x.v.abs() + x.e, win)
    return E(_conv(x.v, win), _conv(x.e, win) + (2 * w + 3) * U * A + TINY)


def ssim_maps(mom):
    """the five moments (E) -> S, p = dS/dmu1 (the e maps held fixed), q = dS/de11, r = dS/de12"""
    mu1, mu2, e11, e22, e12 = mom
    ab, aa, bb = mu1 * mu2, mu1 * mu1, mu2 * mu2
    n1 = ab.twice() + C1
    n2 = (e12 - ab).twice() + C2
    d1 = (aa + bb) + C1
    d2 = ((e11 - aa) + (e22 - bb)) + C2
    den = d1 * d2
    S = (n1 * n2) / den
    p = (mu2.twice() * (n2 - n1)) / den + (mu1.twice() * S) * (E.exact(1.0) / d2 - E.exact(1.0) / d1)
    return S, p, -(S / d2), n1.twice() / den


def ssim_grad(x, y, p, q, r, taps, g_loss=1.0, scale=1.0):
    """((G*p) + 2 x (G*q) + y (G*r)) g_loss scale / numel"""
    kk = (E.exact(g_loss) * E.const(scale)) / E.exact(float(x.v.numel()))
    return ((gfilter(p, taps) + x.twice() * gfilter(q, taps)) + y * gfilter(r, taps)) * kk


def ssim(pred, gt, taps, g_loss=1.0, scale=1.0):
    """pred, gt: (3, H, W) fp32 (or float64) images -> dict: the five moments, S, p, q, r, ssim, gimg = d (scale ssim) / d pred * g_loss
    (each an E)."""
    x, y = E.exact(pred), E.exact(gt)
    mom = [gfilter(x, taps), gfilter(y, taps), gfilter(x * x, taps), gfilter(y * y, taps), gfilter(x * y, taps)]
    S, p, q, r = ssim_maps(mom)
    mean = E(S.v.mean(), S.e.mean())
    mean = mean._round(mean.v, mean.e)                                   # the float64 mean, rounded to fp32 once
    return {'mom': mom, 'S': S, 'p': p, 'q': q, 'r': r, 'ssim': mean, 'gimg': ssim_grad(x, y, p, q, r, taps, g_loss, scale)}


def tv(pred, gt, mask_gt, g_loss=1.0, scale=1.0):
    """pred, gt: (3, H, W); mask_gt (H, W) bool -> dict: eps_x, eps_y, k_x, k_y, mean_x, mean_y, tv (E; NaN where a selection is empty),
    gimg = d (scale tv) / d pred * g_loss (E: elements whose relu decision is within its bound carry the whole term as bound)."""
    x, y = E.exact(pred), E.exact(gt)
    m = mask_gt.bool()
    out = {}
    gv, ge = torch.zeros_like(x.v), torch.zeros_like(x.v)
    means = []
    for name, a, b, ya, yb, sel, lo, hi in (('x', x.sel((slice(None), slice(0, -1))), x.sel((slice(None), slice(1, None))),
                                             y.sel((slice(None), slice(0, -1))), y.sel((slice(None), slice(1, None))), m[:-1, :],
                                             (slice(None), slice(0, -1)), (slice(None), slice(1, None))),
                                            ('y', x.sel((slice(None), slice(None), slice(0, -1))), x.sel((slice(None), slice(None), slice(1, None))),
                                             y.sel((slice(None), slice(None), slice(0, -1))), y.sel((slice(None), slice(None), slice(1, None))),
                                             m[:, :-1], (slice(None), slice(None), slice(0, -1)), (slice(None), slice(None), slice(1, None)))):
        dt = ya - yb
        dt = dt * dt
        eps = E(dt.v.max(), dt.e.max())
        d = a - b
        t = d * d - eps
        k = float(sel.sum())
        selc = sel[None].expand_as(t.v)
        s = E(torch.where(selc, t.v.clamp(min=0.0), 0.0).sum(), torch.where(selc, t.e, 0.0).sum())
        mean = E(s.v / (3.0 * k) if k else torch.tensor(float('nan'), dtype=F64), s.e / (3.0 * k) if k else 0.0)
        mean = mean._round(mean.v, mean.e) if k else mean
        out['eps_' + name], out['k_' + name], out['mean_' + name] = eps, k, mean
        means.append(mean)
        if k:
            c = (E.exact(g_loss) * E.const(scale)) / E.exact(3.0 * k)
            term = c * d
            on, maybe = selc & (t.v > t.e), selc & (t.v.abs() <= t.e)
            tvv, tve = torch.where(on, term.v, 0.0), torch.where(on, term.e, 0.0) + torch.where(maybe, term.v.abs() + term.e, 0.0)
            gv[lo] += tvv
            gv[hi] -= tvv
            ge[lo] += tve
            ge[hi] += tve
    total = E((means[0].v + means[1].v) / 2.0, (means[0].e + means[1].e) / 2.0)
    out['tv'] = total._round(total.v, total.e)
    out['gimg'] = E(gv, ge + 4 * U * (gv.abs() + ge) + TINY)                  # up to four terms added in fp32
    return out


def rays(img, mask):
    """(C, H, W) -> the (n, C) rows of the set mask bytes"""
    return img.reshape(img.shape[0], -1)[:, mask.reshape(-1).bool()].t()
