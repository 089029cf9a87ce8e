"""Checker only: a float64 restatement (with an fp32 mode) of the perceptual image term — invr.losses.PerceptualLoss on the patch
assembled from mask_at_box — one layer at a time, every value with its absolute-value companion A (the same sum with absolute
values) and its summand count c, so that an fp32 evaluation of that ONE layer is held to (c + 4) 2^-24 A + c 2^-126.

The gradient of this loss is piecewise constant in ~1.7 M ReLU / sign / pool decisions; two independent evaluations flip a few of
them and each flip moves a 14 x 14 neighbourhood of the gradient.  So the backward here takes its decisions as INPUTS (`Decisions`):
from the same float64 run (tests/test_perceptual_reference_cpu.py) or from the stored values of the kernel under test
(tests/test_gpu_perceptual.py)."""
import torch
import torch.nn.functional as F

CIN, COUT = (3, 64, 64, 128), (64, 64, 128, 128)
U24, TINY = 2.0 ** -24, 2.0 ** -126


def make_weights(seed):
    """Seeded N(0, 2 / fan_in) weights and N(0, 0.05^2) biases of the four convolutions (fp32, torch's (out, in, 3, 3))."""
    g = torch.Generator().manual_seed(900 + seed)
    ws = [torch.randn(o, i, 3, 3, generator=g) * (2.0 / (9 * i)) ** 0.5 for i, o in zip(CIN, COUT)]
    bs = [torch.randn(o, generator=g) * 0.05 for o in COUT]
    return ws, bs


def assemble(values, mask, H, W):
    """zeros (3, H, W); img[:, mask] = values (n, 3) in row-major mask order."""
    img = torch.zeros(H * W, 3, dtype=values.dtype)
    img[mask.reshape(-1).bool()] = values
    return img.reshape(H, W, 3).permute(2, 0, 1).contiguous()


def bound(c, A):
    return (c + 4) * U24 * A + c * TINY


def conv_fwd(x, w, b, dtype=torch.float64):
    """x (N, Cin, H, W), w, b -> (pre-activation, A, c) of the zero-padded 3x3 convolution in `dtype`."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    return F.conv2d(x, w, b, padding=1), F.conv2d(x.abs(), w.abs(), b.abs(), padding=1), 9 * w.shape[1] + 1


def conv_bwd(g, w, dtype=torch.float64):
    """g (N, Cout, H, W) arriving at the convolution's output -> (data gradient, A, c)."""
    g, w = g.to(dtype), w.to(dtype)
    return F.conv_transpose2d(g, w, padding=1), F.conv_transpose2d(g.abs(), w.abs(), padding=1), 9 * w.shape[0]


def pool(x):
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    v = x[..., :2 * h, :2 * w]
    return torch.maximum(torch.maximum(v[..., 0::2, 0::2], v[..., 0::2, 1::2]), torch.maximum(v[..., 1::2, 0::2], v[..., 1::2, 1::2]))


def pool_first(x):
    """-> int64 (..., h, w): position 0..3 (row-major in the 2x2 window) of the FIRST maximum."""
    h, w = x.shape[-2] // 2, x.shape[-1] // 2
    v = x[..., :2 * h, :2 * w]
    win = torch.stack([v[..., 0::2, 0::2], v[..., 0::2, 1::2], v[..., 1::2, 0::2], v[..., 1::2, 1::2]], -1)
    return (win == win.max(-1, keepdim=True)[0]).to(torch.int64).argmax(-1)          # argmax of 0/1: torch returns the first 1


def pool_route(gp, first, H, W):
    """The pool's backward: gp (C, h, w) sent to position `first` of each window; zeros elsewhere (and in an odd last row / column)."""
    out = torch.zeros(gp.shape[:-2] + (H, W), dtype=gp.dtype)
    h, w = gp.shape[-2:]
    for k in range(4):
        out[..., k // 2:2 * h:2, k % 2:2 * w:2] = torch.where(first == k, gp, torch.zeros_like(gp))
    return out


def sign(d):
    return torch.sign(d)


def forward(ws, bs, img_p, img_t, dtype=torch.float64):
    """-> dict: activations a11, a12, pool, a21, a22 (2, C, H, W) of [predicted, target], the four means l1, l2, li, mse and the loss,
    all in `dtype` with torch's order of operations for the loss."""
    x = torch.stack([img_p, img_t]).to(dtype)
    r = {'img': x}
    r['a11'] = torch.relu(conv_fwd(x, ws[0], bs[0], dtype)[0])
    r['a12'] = torch.relu(conv_fwd(r['a11'], ws[1], bs[1], dtype)[0])
    r['pool'] = pool(r['a12'])
    r['a21'] = torch.relu(conv_fwd(r['pool'], ws[2], bs[2], dtype)[0])
    r['a22'] = torch.relu(conv_fwd(r['a21'], ws[3], bs[3], dtype)[0])
    r['l1'] = (r['a12'][0] - r['a12'][1]).abs().mean()
    r['l2'] = (r['a22'][0] - r['a22'][1]).abs().mean()
    r['li'] = (x[0] - x[1]).abs().mean()
    r['mse'] = ((x[0] - x[1]) ** 2).mean()
    r['loss'] = (r['l1'] + r['l2']) / 2.0 + r['li'] + r['mse']
    # the loss's own companion: every mean is a sum of non-negative terms, so A = the loss; summands of the longest chain
    r['A'] = r['loss'].abs()
    r['c'] = sum(9 * c + 1 for c in CIN) + max(r['a12'][0].numel(), 1)
    return r


class Decisions:
    """Every discrete choice of the backward: ReLU masks m11, m12, m21, m22 (bool, predicted image), sign fields s12, s22, simg
    (-1 / 0 / 1) and the pool's first-maximum position (int64)."""

    def __init__(self, m11, m12, m21, m22, s12, s22, simg, first):
        self.m11, self.m12, self.m21, self.m22, self.s12, self.s22, self.simg, self.first = m11, m12, m21, m22, s12, s22, simg, first

    @staticmethod
    def of(r):
        """From stored activations / features r (keys img, a11, a12, a21, a22 of shape (2, C, H, W)) — torch's rules."""
        return Decisions(r['a11'][0] > 0, r['a12'][0] > 0, r['a21'][0] > 0, r['a22'][0] > 0, sign(r['a12'][0] - r['a12'][1]),
                         sign(r['a22'][0] - r['a22'][1]), sign(r['img'][0] - r['img'][1]), pool_first(r['a12'][0]))


def backward(ws, img_p, img_t, dec, g_loss=1.0, dtype=torch.float64):
    """The whole backward to the predicted image with the decisions `dec` -> dict of the gradient arriving at each layer's output
    (g22, g21, gpool, g12, g11, gimg) with gimg's companion A (propagated through the chain) and its summand count c."""
    H, W = img_p.shape[-2:]
    t = lambda v: torch.as_tensor(v, dtype=dtype)
    n1, n2, ni = dec.s12.numel(), dec.s22.numel(), dec.simg.numel()
    r = {}
    r['g22'] = t(g_loss) / (2 * n2) * dec.s22.to(dtype)
    r['g21'] = conv_bwd((r['g22'] * dec.m22)[None], ws[3], dtype)[0][0]
    A = conv_bwd((r['g22'].abs() * dec.m22)[None], ws[3], dtype)[1][0]
    r['gpool'] = conv_bwd((r['g21'] * dec.m21)[None], ws[2], dtype)[0][0]
    A = conv_bwd((A * dec.m21)[None], ws[2], dtype)[1][0]
    k1 = t(g_loss) / (2 * n1)
    r['g12'] = pool_route(r['gpool'], dec.first, H, W) + k1 * dec.s12.to(dtype)
    A = pool_route(A, dec.first, H, W) + k1.abs() * dec.s12.abs().to(dtype)
    r['g11'] = conv_bwd((r['g12'] * dec.m12)[None], ws[1], dtype)[0][0]
    A = conv_bwd((A * dec.m12)[None], ws[1], dtype)[1][0]
    d = (img_p - img_t).to(dtype)
    r['gimg'] = conv_bwd((r['g11'] * dec.m11)[None], ws[0], dtype)[0][0] + t(g_loss) / ni * dec.simg.to(dtype) + t(g_loss) * 2 / ni * d
    r['A'] = conv_bwd((A * dec.m11)[None], ws[0], dtype)[1][0] + (t(g_loss) / ni).abs() * dec.simg.abs().to(dtype) + (t(g_loss) * 2 / ni * d).abs()
    r['c'] = sum(9 * c for c in COUT) + 4
    return r
