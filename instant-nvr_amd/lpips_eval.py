"""LPIPS v0.1, net='vgg' (spatial=False, eval mode), of two (H,W,3) float32 images in [0, 1] on the device: `LpipsVgg` holds the packed
weights of include/invr_lpips.h (csrc/k_lpips.hip) and a grow-only workspace per (device, stream).  It computes what
lpips.LPIPS(net='vgg')(pred, gt) computes WITHOUT normalize=True, which is how the reference's evaluator calls it
(lib/evaluators/if_nerf.py:118-122): float32 features from exact-fp32 matrix products, the distance in float64; the same inputs give
the same bits in every run, nothing is read back and nothing synchronises.

No weights ship with this package.  They come from tensors, from a module that is recognisably the lpips package's network
(`from_module`), or from the two files that package loads (`from_files`); `random(seed)` is for tests and tools."""
import ctypes as C

import torch
from torch import nn

from . import _abi

CIN, COUT, TAPS = _abi.LPIPS_CIN, _abi.LPIPS_COUT, _abi.LPIPS_TAPS
SHIFT = (-.030, -.088, -.188)          # lpips.ScalingLayer
SCALE = (.458, .449, .450)
VGG16_CONVS = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)          # torchvision vgg16().features indices of the 13 convolutions


def random_tensors(seed):
    """Seeded stand-in weights (fp32, CPU): N(0, 2 / fan_in) convolutions (He), N(0, 0.05^2) biases, lin = U[0, 1) / C (non-negative,
    as the trained ones are) -> (conv_w[13], conv_b[13], lin_w[5])."""
    g = torch.Generator().manual_seed(1600 + int(seed))
    conv_w = [torch.randn(o, i, 3, 3, generator=g) * (2.0 / (9 * i)) ** 0.5 for i, o in zip(CIN, COUT)]
    conv_b = [torch.randn(o, generator=g) * 0.05 for o in COUT]
    lin_w = [torch.rand(COUT[l], generator=g) / COUT[l] for l in TAPS]
    return conv_w, conv_b, lin_w


def module_tensors(m):
    """(conv_w, conv_b, lin_w, shift, scale) of a module that is recognisably lpips.LPIPS(net='vgg') — 13 3x3 stride-1 zero-padded
    `Conv2d`s with bias of the VGG16 plan under `.net`, five bias-free 1x1 `Conv2d` C -> 1 under `lin0` .. `lin4`, and
    `scaling_layer.shift` / `.scale` of 3 values — else None."""
    net, sl = getattr(m, 'net', None), getattr(m, 'scaling_layer', None)
    if not isinstance(net, nn.Module) or sl is None:
        return None
    convs = [c for c in net.modules() if isinstance(c, nn.Conv2d)]
    if len(convs) != 13:
        return None
    for c, i, o in zip(convs, CIN, COUT):
        if not (tuple(c.weight.shape) == (o, i, 3, 3) and c.bias is not None and tuple(c.stride) == (1, 1) and tuple(c.padding) == (1, 1)
                and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.padding_mode == 'zeros'):
            return None
    lins = []
    for k, l in enumerate(TAPS):
        lin = getattr(m, 'lin%d' % k, None)
        if not isinstance(lin, nn.Module):
            return None
        cs = [c for c in lin.modules() if isinstance(c, nn.Conv2d)]
        if len(cs) != 1 or tuple(cs[0].weight.shape) != (1, COUT[l], 1, 1) or cs[0].bias is not None or tuple(cs[0].stride) != (1, 1):
            return None
        lins.append(cs[0].weight.reshape(-1))
    shift, scale = getattr(sl, 'shift', None), getattr(sl, 'scale', None)
    if not (torch.is_tensor(shift) and torch.is_tensor(scale) and shift.numel() == 3 and scale.numel() == 3):
        return None
    return [c.weight for c in convs], [c.bias for c in convs], lins, shift.reshape(-1), scale.reshape(-1)


def _load(path):
    sd = torch.load(path, map_location='cpu')
    if not hasattr(sd, 'keys'):
        raise ValueError('%s does not hold a state dict (got %s)' % (path, type(sd).__name__))
    return sd


def file_tensors(vgg16_path, lin_path):
    """(conv_w, conv_b, lin_w) from a torchvision VGG16 state dict (features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.weight / .bias) and
    the lpips package's vgg.pth (lin{k}.model.1.weight).  Missing keys raise KeyError with the list of keys found."""
    vgg, lin = _load(vgg16_path), _load(lin_path)

    def need(sd, keys, path):
        missing = [k for k in keys if k not in sd]
        if missing:
            raise KeyError('%s: missing %s; keys found: %s' % (path, missing, sorted(sd.keys())))
        return [sd[k] for k in keys]
    conv_w = need(vgg, ['features.%d.weight' % i for i in VGG16_CONVS], vgg16_path)
    conv_b = need(vgg, ['features.%d.bias' % i for i in VGG16_CONVS], vgg16_path)
    lin_w = need(lin, ['lin%d.model.1.weight' % k for k in range(5)], lin_path)
    return conv_w, conv_b, [t.reshape(-1) for t in lin_w]


def _aligned(nbytes, device):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


class LpipsVgg:
    def __init__(self, packed):
        self.packed = packed
        self.device = packed.device
        self._ws = {}                    # stream -> workspace (uint8, 256-byte aligned), grow-only

    @classmethod
    def from_tensors(cls, conv_w, conv_b, lin_w, shift=None, scale=None, device=None):
        """13 (out, in, 3, 3) weights, 13 (out) biases, five lin weights of C values each (any shape), on any device."""
        if len(conv_w) != 13 or len(conv_b) != 13 or len(lin_w) != 5:
            raise ValueError('LpipsVgg: 13 convolution weights, 13 biases and 5 lin weights expected (got %d, %d, %d)'
                             % (len(conv_w), len(conv_b), len(lin_w)))
        for l, (w, b) in enumerate(zip(conv_w, conv_b)):
            if tuple(w.shape) != (COUT[l], CIN[l], 3, 3) or tuple(b.shape) != (COUT[l],):
                raise ValueError('LpipsVgg: convolution %d has weight %r / bias %r, the VGG16 plan has %r / %r'
                                 % (l, tuple(w.shape), tuple(b.shape), (COUT[l], CIN[l], 3, 3), (COUT[l],)))
        for k, t in enumerate(lin_w):
            if t.numel() != COUT[TAPS[k]]:
                raise ValueError('LpipsVgg: lin%d has %d weights, its tap has %d channels' % (k, t.numel(), COUT[TAPS[k]]))
        if device is None:
            device = conv_w[0].device if conv_w[0].is_cuda else torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        to = lambda t: torch.as_tensor(t, dtype=torch.float32).detach().to(device=device, dtype=torch.float32).contiguous()
        shift = to(SHIFT if shift is None else shift).reshape(-1)
        scale = to(SCALE if scale is None else scale).reshape(-1)
        return cls(_abi.lpips_pack([to(t) for t in conv_w], [to(t) for t in conv_b], [to(t).reshape(-1) for t in lin_w], shift, scale))

    @classmethod
    def from_module(cls, m, device=None):
        """An LpipsVgg of a module module_tensors() recognises (on the module's device unless `device` says otherwise), else None."""
        t = module_tensors(m)
        if t is None:
            return None
        return cls.from_tensors(*t, device=device if device is not None else (t[0][0].device if t[0][0].is_cuda else None))

    @classmethod
    def from_files(cls, vgg16_path, lin_path, device=None):
        return cls.from_tensors(*file_tensors(vgg16_path, lin_path), device=device)

    @classmethod
    def random(cls, seed, device=None):
        return cls.from_tensors(*random_tensors(seed), device=device)

    def _workspace(self, nbytes):
        key = _abi.stream_ptr().value
        have = self._ws.get(key)
        if have is None or have.numel() < nbytes:          # grow-only: the byte count is monotone in H and W
            have = self._ws[key] = _aligned(nbytes, self.device)
        return have

    def out8(self, img_pred, img_gt):
        """-> 8 doubles on the device: {lpips, layer_0 .. layer_4, 0, 0} of two (H,W,3) float32 device images."""
        if img_pred.dim() != 3 or img_pred.shape[2] != 3 or img_gt.shape != img_pred.shape:
            raise ValueError('LpipsVgg: two (H,W,3) images expected, got %r and %r' % (tuple(img_pred.shape), tuple(img_gt.shape)))
        if img_pred.device != self.device or img_gt.device != self.device:
            raise ValueError('LpipsVgg: the weights are on %s, the images on %s and %s' % (self.device, img_pred.device, img_gt.device))
        H, W = int(img_pred.shape[0]), int(img_pred.shape[1])
        L = _abi.lib()
        nbytes = L.invr_lpips_workspace_bytes(H, W, 0)
        if nbytes == 0:
            raise ValueError('LpipsVgg: H, W must be in [16, 2048] (got %d x %d)' % (H, W))
        ws = self._workspace(nbytes)
        out = torch.empty(8, dtype=torch.float64, device=self.device)
        a, b = _abi.f32c(img_pred), _abi.f32c(img_gt)          # (both alive until the launch: two temporaries must not share a block)
        _abi.check(L.invr_lpips_fwd(_abi.ptr(self.packed), _abi.ptr(a), _abi.ptr(b), H, W, 0,
                                    _abi.ptr(ws, torch.uint8), C.c_size_t(ws.numel()), _abi.ptr(out, torch.float64), _abi.stream_ptr()))
        return out

    def __call__(self, img_pred, img_gt):
        """-> the device double lpips(img_pred, img_gt) (0-dim)"""
        return self.out8(img_pred, img_gt)[0]
