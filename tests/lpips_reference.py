"""Checker only: LPIPS v0.1 net='vgg' (spatial=False, eval mode, no normalize) restated in torch on the CPU in float64, with an fp32
mode of the same code — the network of include/invr_lpips.h one stage at a time, so that the kernels (csrc/k_lpips.hip) can be held
layer by layer to the float64 value of their OWN stored input.  bound(c, A) is tests/perceptual_reference.py's."""
import torch
import torch.nn.functional as F

from tests.perceptual_reference import bound, conv_fwd, pool          # noqa: F401  (the same rules, stated once)

CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
BLOCK = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
TAPS = (1, 3, 6, 9, 12)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .449, .450)
EPS = float(torch.tensor(1e-10, dtype=torch.float32))          # (double)1e-10f
U53 = 2.0 ** -53


def make_weights(seed):
    """The rule of invr.lpips_eval.random_tensors, restated: N(0, 2 / fan_in) convolutions, N(0, 0.05^2) biases, lin = U[0, 1) / C."""
    g = torch.Generator().manual_seed(1600 + seed)
    conv_w = [torch.randn(o, i, 3, 3, generator=g) * (2.0 / (9 * i)) ** 0.5 for i, o in zip(CIN, COUT)]
    conv_b = [torch.randn(o, generator=g) * 0.05 for o in COUT]
    lin_w = [torch.rand(COUT[l], generator=g) / COUT[l] for l in TAPS]
    return conv_w, conv_b, lin_w


def scale_layer(img, dtype=torch.float64):
    """(H, W, 3) -> planar (3, H, W): (img - shift) / scale in `dtype`, shift and scale being the fp32 constants."""
    sh = torch.tensor(SHIFT, dtype=torch.float32).to(dtype)
    sc = torch.tensor(SCALE, dtype=torch.float32).to(dtype)
    return ((img.to(dtype) - sh) / sc).permute(2, 0, 1).contiguous()


def distance(feat, lin, dtype=torch.float64):
    """feat (2, C, h, w), lin (C) -> (layer value, A): A = the same mean with (|n0| + |n1|)^2 in the place of (n0 - n1)^2 and |lin|."""
    x = feat.to(dtype)
    lw = lin.to(dtype).reshape(-1, 1, 1)
    n = x / ((x * x).sum(1, keepdim=True).sqrt() + torch.tensor(EPS, dtype=dtype))
    hw = x.shape[2] * x.shape[3]
    d = (lw * (n[0] - n[1]) ** 2).sum(0)
    A = (lw.abs() * (n[0].abs() + n[1].abs()) ** 2).sum(0)
    return d.sum() / hw, A.sum() / hw


def distance_rel(C, pixels):
    """Bound, in units of 2^-53 A, on the difference of two float64 evaluations of distance() that differ in the order of their sums.
    With u = 2^-53, to first order and per evaluation: S = sum_c x^2 of non-negative terms carries C u (a product and C - 1
    additions per term at most); sqrt halves it and adds u, + eps adds u, the quotient adds u: |dn| <= (C / 2 + 3) u |n|.  Two
    evaluations differ by twice that, (C + 6) u |n|.  The difference n0 - n1 then differs by (C + 6) u (|n0| + |n1|) + 2 u |n0 - n1|
    <= (C + 8) u (|n0| + |n1|); its square by 2 |n0 - n1| times that + 2 u (n0 - n1)^2 <= (2 C + 18) u (|n0| + |n1|)^2; the product
    with lin adds 2 u, the sum over C non-negative terms 2 C u, the sum over the pixels in any order 2 pixels u, the division by
    h w 2 u: (4 C + 2 pixels + 22) u A, rounded up to 4 C + 2 pixels + 32."""
    return 4 * C + 2 * pixels + 32


def forward(weights, img_p, img_t, dtype=torch.float64):
    """(H, W, 3) images -> dict: scaled (2, 3, H, W), act[13], pool[4], layer[5] and lpips, all in `dtype`."""
    conv_w, conv_b, lin_w = weights
    x = torch.stack([scale_layer(img_p, dtype), scale_layer(img_t, dtype)])
    r = {'scaled': x, 'act': [], 'pool': [], 'layer': []}
    for l in range(13):
        if l > 0 and BLOCK[l] != BLOCK[l - 1]:
            x = pool(x)
            r['pool'].append(x)
        x = torch.relu(F.conv2d(x, conv_w[l].to(dtype), conv_b[l].to(dtype), padding=1))
        r['act'].append(x)
        if l in TAPS:
            r['layer'].append(distance(x, lin_w[TAPS.index(l)], dtype)[0])
    v = r['layer'][0]
    for k in range(1, 5):
        v = v + r['layer'][k]
    r['lpips'] = v
    return r


# ---- a module with the lpips package's attribute names (what invr.lpips_eval.module_tensors recognises) ----------------------------------
class ScalingLayer(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer('shift', torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer('scale', torch.tensor(SCALE)[None, :, None, None])

    def forward(self, x):
        return (x - self.shift) / self.scale


class NetLinLayer(torch.nn.Module):
    def __init__(self, c, bias=False):
        super().__init__()
        self.model = torch.nn.Sequential(torch.nn.Dropout(), torch.nn.Conv2d(c, 1, 1, stride=1, padding=0, bias=bias))

    def forward(self, x):
        return self.model(x)


class Vgg16(torch.nn.Module):
    """slice1 .. slice5 holding torchvision's vgg16().features layers under their indices, as the package's pretrained_networks.vgg16"""

    def __init__(self, cin=CIN, cout=COUT):
        super().__init__()
        nn = torch.nn
        for k in range(5):
            seq = nn.Sequential()
            if k > 0:
                seq.add_module('pool', nn.MaxPool2d(2, 2))
            for l in range(13):
                if BLOCK[l] == k:
                    seq.add_module('conv%d' % l, nn.Conv2d(cin[l], cout[l], 3, padding=1))
                    seq.add_module('relu%d' % l, nn.ReLU(inplace=False))
            setattr(self, 'slice%d' % (k + 1), seq)

    def forward(self, x):
        outs = []
        for k in range(5):
            x = getattr(self, 'slice%d' % (k + 1))(x)
            outs.append(x)
        return outs


class Lpips(torch.nn.Module):
    """lpips.LPIPS(net='vgg', spatial=False) restated with its attribute names: net, scaling_layer, lin0 .. lin4."""

    def __init__(self, weights=None, cin=CIN, cout=COUT, lin_bias=False, scaling=True):
        super().__init__()
        self.net = Vgg16(cin, cout)
        if scaling:
            self.scaling_layer = ScalingLayer()
        for k, l in enumerate(TAPS):
            setattr(self, 'lin%d' % k, NetLinLayer(cout[l], lin_bias))
        if weights is not None:
            conv_w, conv_b, lin_w = weights
            convs = [m for m in self.net.modules() if isinstance(m, torch.nn.Conv2d)]
            with torch.no_grad():
                for c, w, b in zip(convs, conv_w, conv_b):
                    c.weight.copy_(w)
                    c.bias.copy_(b)
                for k in range(5):
                    getattr(self, 'lin%d' % k).model[1].weight.copy_(lin_w[k].reshape(1, -1, 1, 1))

    def forward(self, in0, in1):
        f0, f1 = self.net(self.scaling_layer(in0)), self.net(self.scaling_layer(in1))
        val = 0
        for k in range(5):
            n0 = f0[k] / (torch.sqrt(torch.sum(f0[k] ** 2, dim=1, keepdim=True)) + 1e-10)
            n1 = f1[k] / (torch.sqrt(torch.sum(f1[k] ** 2, dim=1, keepdim=True)) + 1e-10)
            val = val + getattr(self, 'lin%d' % k).model[1]((n0 - n1) ** 2).mean([2, 3], keepdim=True)
        return val
