"""Regenerates tests/golden/imgloss_small.npz from the reference's own SSIM and TVImageLoss:

    python tests/golden/make_golden_imgloss.py /path/to/reference

The two classes are loaded by file path (lib/utils/loss_utils.py, lib/train/trainers/loss/tv_image_loss.py import nothing but torch
and numpy) and run on a few seeded patches assembled through a mask_at_box with holes, exactly as inb_trainer.py:196-226 does.  Arrays
only are recorded, per case `<H>x<W>`:

    mask (H*W uint8), occ (n uint8), ssim_pred / ssim_gt / tv_pred / tv_gt (n, 3) fp32 rays,
    ssim_f32, tv_f32            the reference's value in fp32
    ssim_f64, tv_f64            the same code in float64
    ssim_grad_f32, tv_grad_f32  d value / d pred rays (n, 3), fp32 autograd
    ssim_grad_f64, tv_grad_f64  the same in float64
and once `taps11`, the reference's gaussian(11, 1.5).

TV: the target is dark (rays in [0, 0.3]) and the prediction spans [0, 1], so that the prediction is rougher than the target's largest
step (eps, which the zero-filled holes of the target push up to ~0.09): 52-54 % of the selected relu terms are active (printed per case,
recorded as tv_active)."""
import importlib.util
import os
import sys

import numpy as np
import torch

CASES = ((7, 9), (16, 16), (24, 40))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def patch(values, mask, H, W):
    img = torch.zeros((H, W, values.shape[-1]), dtype=values.dtype)
    img[mask.reshape(H, W)] = values
    return img


def main(ref):
    lu = load(os.path.join(ref, 'lib/utils/loss_utils.py'), 'ref_loss_utils')
    tvm = load(os.path.join(ref, 'lib/train/trainers/loss/tv_image_loss.py'), 'ref_tv_image_loss')
    out = {'taps11': lu.gaussian(11, 1.5).numpy()}
    for H, W in CASES:
        g = torch.Generator().manual_seed(1000 * H + W)
        mask = torch.rand(H * W, generator=g) < 0.8
        n = int(mask.sum())
        occ = torch.rand(n, generator=g) < 0.7
        base = torch.rand(n, 3, generator=g)
        rec = {'mask': mask.to(torch.uint8).numpy(), 'occ': occ.to(torch.uint8).numpy(),
               'ssim_pred': base, 'ssim_gt': (base + 0.1 * torch.randn(n, 3, generator=g)).clamp(0, 1),
               'tv_pred': torch.rand(n, 3, generator=g), 'tv_gt': 0.3 * torch.rand(n, 3, generator=g)}
        mask_gt = patch(occ[:, None], mask, H, W)[..., 0]
        for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
            pred = rec['ssim_pred'].detach().clone().to(dt).requires_grad_(True)
            ssim = lu.SSIM(window_size=11)
            v = ssim(patch(pred, mask, H, W).permute(2, 0, 1)[None], patch(rec['ssim_gt'].to(dt), mask, H, W).permute(2, 0, 1)[None])
            v.backward()
            rec['ssim_' + tag], rec['ssim_grad_' + tag] = v.detach().numpy(), pred.grad.numpy()
            pred = rec['tv_pred'].detach().clone().to(dt).requires_grad_(True)
            ip, ig = patch(pred, mask, H, W), patch(rec['tv_gt'].to(dt), mask, H, W)
            v = tvm.TVImageLoss()(ip, ig, mask_gt)
            v.backward()
            rec['tv_' + tag], rec['tv_grad_' + tag] = v.detach().numpy(), pred.grad.numpy()
        with torch.no_grad():
            ip, ig = patch(rec['tv_pred'], mask, H, W), patch(rec['tv_gt'], mask, H, W)
            ax = (torch.square(ip[:-1] - ip[1:]) > torch.square(ig[:-1] - ig[1:]).max())[mask_gt[:-1, :]]
            ay = (torch.square(ip[:, :-1] - ip[:, 1:]) > torch.square(ig[:, :-1] - ig[:, 1:]).max())[mask_gt[:, :-1]]
            share = float(torch.cat([ax.reshape(-1), ay.reshape(-1)]).float().mean())
        rec['tv_active'] = np.float64(share)
        print('%dx%d: %d rays, ssim %.7f (fp32 - float64 %.2e), tv %.7g (fp32 - float64 %.2e), active relu terms %.1f %%'
              % (H, W, n, float(rec['ssim_f64']), float(rec['ssim_f32']) - float(rec['ssim_f64']), float(rec['tv_f64']),
                 float(rec['tv_f32']) - float(rec['tv_f64']), 100 * share))
        for k, a in rec.items():
            out['%dx%d/%s' % (H, W, k)] = a.numpy() if torch.is_tensor(a) else a
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'imgloss_small.npz'), **out)


if __name__ == '__main__':
    main(sys.argv[1])
