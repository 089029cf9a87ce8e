"""Image-space loss of the reference's LPIPS branch (lib/train/trainers/loss/perceptual_loss.py:6-68): L1 on the relu1_2 /
relu2_2 activations of a frozen VGG19 + L1 + L2 on the image.

The reference builds the VGG through torchvision and downloads ImageNet weights; neither torchvision nor a network is
available on this image, so the feature stack is restated here as plain `nn.Conv2d`s with torchvision's own
`vgg19().features` indices and state_dict keys ('0.weight', '2.weight', '5.weight', '7.weight'): a torchvision
checkpoint (full model or its `.features`) loads directly.  Without weights the constructor refuses to build a loss
network (training against random features would silently optimise a different objective) unless `allow_random=True`
(tests of the patch re-assembly / plumbing only).

`FusedPerceptual` is the HIP form of the same loss (csrc/k_perceptual.hip, include/invr_perceptual.h) for any module that is
recognisably this network: the packed weight image, rebuilt when the weights change, and the workspace of its intermediates.

`SSIM` and `TVImageLoss` are the reference's other two image terms (lib/utils/loss_utils.py:7-63, lib/train/trainers/loss/tv_image_loss.py)
as torch ops, for hosts that have neither class; `FusedImageTerms` is what their HIP form (csrc/k_imgloss.hip, include/invr_imgloss.h)
keeps between iterations.
"""
import math

import torch
import torch.nn as nn


class VggRelu12(nn.Module):
    """features[0..8] of torchvision's vgg19: conv3-64, relu, conv64-64, relu (3: "relu1"), maxpool, conv64-128, relu,
    conv128-128, relu (8: "relu2") — perceptual_loss.py:36-47 stops after layer 8."""

    def __init__(self):
        super().__init__()
        self.vgg_layers = nn.Sequential(
            nn.Conv2d(3, 64, 3, padding=1), nn.ReLU(inplace=False), nn.Conv2d(64, 64, 3, padding=1), nn.ReLU(inplace=False),
            nn.MaxPool2d(2, 2), nn.Conv2d(64, 128, 3, padding=1), nn.ReLU(inplace=False), nn.Conv2d(128, 128, 3, padding=1),
            nn.ReLU(inplace=False))
        for p in self.parameters():
            p.requires_grad = False

    def load_torchvision(self, sd):
        """Accepts vgg19().state_dict() ('features.N.*'), vgg19().features.state_dict() ('N.*') or this module's own."""
        own = {}
        for k, v in sd.items():
            k = k[len('features.'):] if k.startswith('features.') else k
            k = k[len('vgg_layers.'):] if k.startswith('vgg_layers.') else k
            if k.split('.')[0] in ('0', '2', '5', '7'):
                own[k] = v
        self.vgg_layers.load_state_dict(own, strict=True)
        return self

    def forward(self, x):
        out = []
        for i, m in enumerate(self.vgg_layers):
            x = m(x)
            if i in (3, 8):
                out.append(x)
        return out


class PerceptualLoss(nn.Module):
    """perceptual_loss.py:45-68: (L1(relu1) + L1(relu2)) / 2 + L1(image) + MSE(image); inputs (1,3,H,W)."""

    def __init__(self, weights=None, allow_random=False):
        super().__init__()
        self.model = VggRelu12()
        if weights is not None:
            sd = torch.load(weights, map_location='cpu') if isinstance(weights, str) else weights
            self.model.load_torchvision(sd)
        elif not allow_random:
            raise RuntimeError('PerceptualLoss needs the VGG19 ImageNet weights (torchvision vgg19 state_dict); pass weights=<path or '
                               'state_dict>.  There is no network on this image to download them.')
        self.model.eval()

    def forward(self, x, target):
        fx, ft = self.model(x[:, 0:3]), self.model(target[:, 0:3])
        feature_loss = ((fx[0] - ft[0]).abs().mean() + (fx[1] - ft[1]).abs().mean()) / 2.0
        return feature_loss + (x - target).abs().mean() + ((x - target) ** 2).mean()


VGG_CONV_INDICES = (0, 2, 5, 7)
VGG_CONV_SHAPES = ((64, 3, 3, 3), (64, 64, 3, 3), (128, 64, 3, 3), (128, 128, 3, 3))


def vgg_convs(module):
    """The four convolutions of a perceptual-loss module that is recognisably the reference's network — this file's PerceptualLoss, or
    any module whose `.model.vgg_layers` holds 3x3 stride-1 zero-padded `Conv2d`s of the four shapes at torchvision's indices 0, 2, 5,
    7 (the reference's own torchvision-built LossNetwork) — else None."""
    layers = getattr(getattr(module, 'model', None), 'vgg_layers', None)
    if layers is None or not isinstance(layers, nn.Sequential) or len(layers) < 9:
        return None
    convs = [layers[i] for i in VGG_CONV_INDICES]
    for c, shape in zip(convs, VGG_CONV_SHAPES):
        if not (isinstance(c, nn.Conv2d) and tuple(c.weight.shape) == shape and c.bias is not None and tuple(c.stride) == (1, 1)
                and tuple(c.padding) == (1, 1) and tuple(c.dilation) == (1, 1) and c.groups == 1 and c.padding_mode == 'zeros'):
            return None
    if not (all(isinstance(layers[i], nn.ReLU) for i in (1, 3, 6, 8)) and isinstance(layers[4], nn.MaxPool2d)):
        return None
    pool = layers[4]
    same = lambda v, k: (tuple(v) if isinstance(v, (tuple, list)) else (v, v)) == (k, k)
    if not (same(pool.kernel_size, 2) and same(pool.stride, 2) and same(pool.padding, 0) and not pool.ceil_mode):
        return None
    return convs


class FusedPerceptual:
    """What the HIP perceptual loss keeps between iterations for one module: the packed weight image (invr_perceptual_pack_weights;
    cached, rebuilt when one of the eight tensors was written to — tensor version counters — reallocated or moved) and the
    workspace of the intermediates (256-byte aligned, grown on demand)."""

    def __init__(self):
        self._key = self._packed = self._ws = self._ws_raw = None
        self.gen = 0                       # hand-outs of the workspace: a backward refuses to run on a buffer a later forward has overwritten

    def packed(self, convs):
        from . import _abi
        tensors = [c.weight for c in convs] + [c.bias for c in convs]
        key = tuple((t.data_ptr(), t._version, str(t.device), t.dtype) for t in tensors)
        if self._key != key:
            self._packed = _abi.perceptual_pack(tensors[:4], tensors[4:], None if self._packed is None or self._packed.device != tensors[0].device
                                                else self._packed)
            self._key = key
        return self._packed

    def workspace(self, H, W, device):
        from . import _abi
        nbytes = int(_abi.lib().invr_perceptual_workspace_bytes(int(H), int(W)))
        if nbytes == 0:
            raise RuntimeError('perceptual loss: patch of %d x %d is outside the supported sizes' % (H, W))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != torch.device(device):
            raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
            off = (-raw.data_ptr()) % 256
            self._ws_raw, self._ws = raw, raw[off:off + nbytes]
        self.gen += 1
        return self._ws


def gaussian_taps(window_size, sigma=1.5):
    """loss_utils.py:7-9 as torch forms it: Python doubles rounded to fp32, an fp32 sum, an fp32 division -> (window_size,) fp32."""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def gaussian_window(window_size, channel):
    """loss_utils.py:11-15: the (channel, 1, w, w) window g g^T."""
    g = gaussian_taps(window_size).unsqueeze(1)
    return g.mm(g.t()).float()[None, None].expand(channel, 1, window_size, window_size).contiguous()


class SSIM(nn.Module):
    """loss_utils.py:17-63: mean SSIM of two (N, C, H, W) images under a Gaussian window of sigma 1.5, zero padding."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average
        self.channel = 1
        self.window = gaussian_window(window_size, self.channel)

    def forward(self, img1, img2):
        channel = img1.shape[1]
        if channel != self.channel or self.window.device != img1.device or self.window.dtype != img1.dtype:
            self.window = gaussian_window(self.window_size, channel).to(device=img1.device, dtype=img1.dtype)
            self.channel = channel
        F = torch.nn.functional
        conv = lambda t: F.conv2d(t, self.window, padding=self.window_size // 2, groups=channel)
        mu1, mu2 = conv(img1), conv(img2)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        sigma1_sq, sigma2_sq, sigma12 = conv(img1 * img1) - mu1_sq, conv(img2 * img2) - mu2_sq, conv(img1 * img2) - mu1_mu2
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
        return ssim_map.mean() if self.size_average else ssim_map.mean(1).mean(1).mean(1)


class TVImageLoss(nn.Module):
    """tv_image_loss.py:11-21: squared differences of neighbouring pixels of the (H, W, 3) prediction beyond the target's largest,
    averaged over the pixels of `mask` (H, W, bool) — NaN when a selection is empty, as there."""

    def forward(self, img_pred, img_gt, mask):
        eps_x = torch.square(img_gt[:-1, :, :] - img_gt[1:, :, :]).max()
        eps_y = torch.square(img_gt[:, :-1, :] - img_gt[:, 1:, :]).max()
        diff_x = torch.relu(torch.square(img_pred[:-1, :, :] - img_pred[1:, :, :]) - eps_x)[mask[:-1, :]].mean()
        diff_y = torch.relu(torch.square(img_pred[:, :-1, :] - img_pred[:, 1:, :]) - eps_y)[mask[:, :-1]].mean()
        return (diff_x + diff_y) / 2.0


IMGLOSS_MAX_SIDE, IMGLOSS_MAX_WINDOW = 2048, 31          # include/invr_imgloss.h


def ssim_window_size(module):
    """The window size of an SSIM module that is recognisably the reference's — this file's SSIM or any module with an odd
    `window_size` <= 31, `size_average` True and, where it holds a `window`, the Gaussian window of that size — else None."""
    w, window = getattr(module, 'window_size', None), getattr(module, 'window', None)
    if not isinstance(module, nn.Module) or not isinstance(w, int) or w < 1 or w > IMGLOSS_MAX_WINDOW or w % 2 == 0:
        return None
    if getattr(module, 'size_average', None) is not True:
        return None
    if window is not None:
        if not torch.is_tensor(window) or window.dim() != 4 or tuple(window.shape[1:]) != (1, w, w):
            return None
        if not torch.equal(window.detach().float().cpu(), gaussian_window(w, window.shape[0])):
            return None
    return w


def is_tv_module(module, host_cls=None):
    """A TV module that is recognisably the reference's: of the host application's class or of this file's."""
    return isinstance(module, TVImageLoss) or (host_cls is not None and type(module) is host_cls)


class FusedImageTerms:
    """What the HIP SSIM / TV terms keep between iterations: the taps (per window size and device), the workspace of the
    intermediates (256-byte aligned, grown on demand) and the count of its hand-outs."""

    def __init__(self):
        self._taps, self._ws, self._ws_raw = {}, None, None
        self.gen = 0                       # hand-outs of the workspace: a backward refuses to run on a buffer a later forward has overwritten

    def taps(self, window_size, device):
        key = (int(window_size), str(torch.device(device)))
        if key not in self._taps:
            self._taps[key] = gaussian_taps(window_size).to(device)
        return self._taps[key]

    def workspace(self, H, W, window_size, device):
        from . import _abi
        nbytes = int(_abi.lib().invr_imgloss_workspace_bytes(int(H), int(W), int(window_size)))
        if nbytes == 0:
            raise RuntimeError('image terms: patch of %d x %d (window %d) is outside the supported sizes' % (H, W, window_size))
        if self._ws is None or self._ws.numel() < nbytes or self._ws.device != torch.device(device):
            raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
            off = (-raw.data_ptr()) % 256
            self._ws_raw, self._ws = raw, raw[off:off + nbytes]
        self.gen += 1
        return self._ws
