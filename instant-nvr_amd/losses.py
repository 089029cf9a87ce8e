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
"""
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
