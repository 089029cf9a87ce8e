"""CPU: the float64 statement of the SSIM / TV image terms (tests/imgloss_reference.py) pinned to the reference's own float64
evaluation recorded in tests/golden/imgloss_small.npz (value and d / d pred per ray), its error bounds shown to cover the reference's
own fp32 evaluation, and invr.losses.SSIM / TVImageLoss / gaussian_taps pinned to the reference's fp32 values."""
import os

import numpy as np
import pytest
import torch

from invr import losses
from invr.trainer import assemble_patch
from tests import imgloss_reference as R

Z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'imgloss_small.npz'))
NAMES = ('7x9', '16x16', '24x40')


def case(name, term):
    H, W = (int(v) for v in name.split('x'))
    t = lambda k: torch.from_numpy(Z['%s/%s' % (name, k)])
    return H, W, t('mask'), t(term + '_pred'), t(term + '_gt'), t('occ')


def test_taps_are_the_references():
    ref = torch.from_numpy(Z['taps11'])
    assert torch.equal(R.gaussian_taps(11), ref) and torch.equal(losses.gaussian_taps(11), ref)
    assert torch.equal(losses.gaussian_window(11, 3)[1, 0], ref[:, None] * ref[None, :])


@pytest.mark.parametrize('name', NAMES)
def test_float64_statement_against_the_golden_ssim(name):
    H, W, mask, pred, gt, _ = case(name, 'ssim')
    ex = R.ssim(R.assemble(pred, mask, H, W), R.assemble(gt, mask, H, W), R.gaussian_taps(11))
    v64, g64 = float(Z[name + '/ssim_f64']), torch.from_numpy(Z[name + '/ssim_grad_f64'])
    assert abs(float(ex['ssim'].v) - v64) <= 1e-13
    assert float((R.rays(ex['gimg'].v, mask) - g64).abs().max()) <= 1e-14
    # the bounds cover the reference's own fp32 evaluation (and are not vacuous: within 2^12 of it)
    dv, dg = abs(float(Z[name + '/ssim_f32']) - v64), (torch.from_numpy(Z[name + '/ssim_grad_f32']).double() - g64).abs()
    assert dv <= float(ex['ssim'].e) <= 4096 * max(dv, 2.0 ** -26)
    assert bool((dg <= R.rays(ex['gimg'].e, mask)).all())


@pytest.mark.parametrize('name', NAMES)
def test_float64_statement_against_the_golden_tv(name):
    H, W, mask, pred, gt, occ = case(name, 'tv')
    mask_gt = R.assemble(occ[:, None], mask, H, W)[0] != 0
    ex = R.tv(R.assemble(pred, mask, H, W), R.assemble(gt, mask, H, W), mask_gt)
    v64, g64 = float(Z[name + '/tv_f64']), torch.from_numpy(Z[name + '/tv_grad_f64'])
    assert abs(float(ex['tv'].v) - v64) <= 1e-15
    assert float((R.rays(ex['gimg'].v, mask) - g64).abs().max()) <= 1e-16
    dv, dg = abs(float(Z[name + '/tv_f32']) - v64), (torch.from_numpy(Z[name + '/tv_grad_f32']).double() - g64).abs()
    assert dv <= float(ex['tv'].e) and bool((dg <= R.rays(ex['gimg'].e, mask)).all())
    assert 0.3 < float(Z[name + '/tv_active']) < 0.7                               # a substantial share of the relu terms is active


@pytest.mark.parametrize('name', NAMES)
def test_losses_modules_give_the_references_fp32_values(name):
    H, W, mask, pred, gt, _ = case(name, 'ssim')
    m = mask.reshape(H, W).bool()
    ip, ig = assemble_patch(pred, m, H, W), assemble_patch(gt, m, H, W)
    v = losses.SSIM(window_size=11)(ip.permute(2, 0, 1)[None], ig.permute(2, 0, 1)[None])
    assert v.dtype == torch.float32 and float(v) == float(Z[name + '/ssim_f32'])
    H, W, mask, pred, gt, occ = case(name, 'tv')
    ip, ig = assemble_patch(pred, m, H, W), assemble_patch(gt, m, H, W)
    mask_gt = assemble_patch(occ.float()[:, None], m, H, W)[..., 0] > 0
    pred_img = ip.clone().requires_grad_(True)
    v = losses.TVImageLoss()(pred_img, ig, mask_gt)
    assert float(v.detach()) == float(Z[name + '/tv_f32'])
    v.backward()
    assert torch.equal(pred_img.grad[m], torch.from_numpy(Z[name + '/tv_grad_f32']))


def test_tv_of_an_empty_selection_is_nan():
    img = torch.rand(4, 5, 3)
    assert torch.isnan(losses.TVImageLoss()(img, img * 0.5, torch.zeros(4, 5, dtype=torch.bool)))
    ex = R.tv(img.permute(2, 0, 1), img.permute(2, 0, 1) * 0.5, torch.zeros(4, 5, dtype=torch.bool))
    assert torch.isnan(ex['tv'].v) and float(ex['gimg'].v.abs().max()) == 0.0


def test_recognition_rules():
    assert losses.ssim_window_size(losses.SSIM(11)) == 11 and losses.ssim_window_size(losses.SSIM(7)) == 7
    assert losses.ssim_window_size(losses.SSIM(12)) is None and losses.ssim_window_size(losses.SSIM(33)) is None
    assert losses.ssim_window_size(losses.SSIM(11, size_average=False)) is None
    other = losses.SSIM(11)
    other.window = other.window * 2.0
    assert losses.ssim_window_size(other) is None and losses.ssim_window_size(torch.nn.Identity()) is None
    assert losses.is_tv_module(losses.TVImageLoss()) and not losses.is_tv_module(torch.nn.Identity())


def test_standalone_wrapper_builds_the_modules_only_when_asked():
    """outside the reference application use_ssim / use_tv_image keep raising; cfg.builtin_image_terms builds invr.losses' modules"""
    from invr.config import make_cfg
    from invr.network import Network
    from invr.trainer import NetworkWrapper
    for flag in ('use_ssim', 'use_tv_image'):
        with pytest.raises(RuntimeError, match='builtin_image_terms'):
            NetworkWrapper(Network(cfg=make_cfg(table_log2=8, **{flag: True})))
    w = NetworkWrapper(Network(cfg=make_cfg(table_log2=8, use_ssim=True, use_tv_image=True, builtin_image_terms=True)))
    assert isinstance(w.ssim_loss, losses.SSIM) and w.ssim_loss.window_size == 11 and isinstance(w.tv_image_loss, losses.TVImageLoss)
    with pytest.raises(RuntimeError, match='use_fourier'):          # the one image term that stays the host application's alone
        NetworkWrapper(Network(cfg=make_cfg(table_log2=8, use_fourier=True, builtin_image_terms=True)))
