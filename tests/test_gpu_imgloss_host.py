"""GPU: the host layer of the HIP SSIM / TV image terms — autograd.TrainLossSsimFn / TrainLossTvFn, losses.FusedImageTerms and a
stand-alone NetworkWrapper with cfg.use_ssim / cfg.use_tv_image on the golden 64 x 64 scene.

  * with cfg.builtin_image_terms the wrapper builds its module from invr.losses when no host application provides one, and trains;
  * loss == regulariser terms + (0.1 ssim_loss | 0.01 tv_loss) + img_loss;
  * the term agrees with the float64 statement of the same rgb_map inside its derived bound (tests/imgloss_reference.py), and so does
    the op-by-op path's;
  * the fused g_rgb, pushed through the render's backward, reproduces the op-by-op path's parameter gradients;
  * cfg.fused_image_terms False, an unrecognised module and an out-of-range side keep the op-by-op path; use_lpips wins over use_ssim.
tests/test_hostsim_imgloss_host_cpu.py runs the same bodies on the CPU wave machine under HOSTSIM_FULL=1."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import imgloss_reference as R             # noqa: E402  (checker only)
from invr import losses                              # noqa: E402
from invr.network import Network                     # noqa: E402
from invr.trainer import NetworkWrapper              # noqa: E402

DEV = 'cuda:0'
FLAG = {'ssim': 'use_ssim', 'tv': 'use_tv_image'}
WEIGHT = {'ssim': 0.1, 'tv': 0.01}


def make(small_setup, **flags):
    cfg, sd, batch, _ = small_setup
    net = Network(cfg=copy.deepcopy(cfg))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()
    for k, v in flags.items():
        setattr(net.cfg, k, v)
    gb = {k: v.to(DEV) for k, v in batch.items()}
    n, S = gb['ray_o'].shape[1], net.cfg.N_samples
    g = torch.Generator().manual_seed(5)
    jitter, noise = torch.rand(n, S, generator=g), torch.rand(n * S * 5, 3, generator=g)
    tb = dict(gb)
    tb['iter_step'] = 2

    def pin(wrap):
        wrap.renderer._jitter = lambda shape, device: jitter.to(device)
        wrap.renderer._pair_noise_dense = lambda rows, device: noise.to(device)[:rows]
        return wrap
    return net, tb, pin


def iteration(wrap, net, tb):
    params = [p for p in net.parameters() if p.requires_grad]
    for p in params:
        p.grad = None
    ret, loss, stats, _ = wrap(tb, split='train')
    ret['rgb_map'].retain_grad()
    loss.backward()
    out = {'ret': ret, 'loss': loss.detach(), 'stats': {k: v.detach() for k, v in stats.items()}, 'grad_fn': {k: v.requires_grad for k, v in stats.items()},
           'g_rgb': ret['rgb_map'].grad.clone(), 'grads': [None if p.grad is None else p.grad.detach().clone() for p in params],
           'error': ret['error'].detach().clone()}
    for p in params:
        p.grad = None
    return out


@pytest.fixture(scope='module', params=('ssim', 'tv'))
def step(request, small_setup):
    """One training iteration of a stand-alone NetworkWrapper with the term on the HIP path, then the same iteration op by op."""
    term = request.param
    net, tb, pin = make(small_setup, builtin_image_terms=True, **{FLAG[term]: True})
    if term == 'tv':                                         # a dark target: the rendered patch is rougher than its largest step, relu terms are active
        tb['rgb'] = tb['rgb'] * 0.02
    wrap = pin(NetworkWrapper(net))                          # no host application: built from invr.losses (cfg.builtin_image_terms)
    fused = iteration(wrap, net, tb)
    gen = wrap._fused_image_terms.gen
    net.cfg.fused_image_terms = False
    plain = iteration(wrap, net, tb)
    net.cfg.fused_image_terms = True
    assert wrap._fused_image_terms.gen == gen                # the switch kept the torch ops
    return {'term': term, 'wrap': wrap, 'net': net, 'tb': tb, 'fused': fused, 'plain': plain,
            'names': [k for k, p in net.named_parameters() if p.requires_grad]}


def test_standalone_wrapper_builds_and_trains(step):
    term, wrap, f = step['term'], step['wrap'], step['fused']
    mod = wrap.ssim_loss if term == 'ssim' else wrap.tv_image_loss
    assert isinstance(mod, losses.SSIM if term == 'ssim' else losses.TVImageLoss)
    assert torch.isfinite(f['loss']) and wrap._fused_image_terms.gen >= 1 and float(f['stats'][term + '_loss']) > 0
    assert not f['grad_fn'][term + '_loss'] and step['plain']['grad_fn'][term + '_loss']          # a statistic of the fused node / a torch-op graph
    assert sum(g is not None and float(g.abs().max()) > 0 for g in f['grads']) >= 20


def test_loss_is_regularisers_plus_term_plus_mse(step):
    term, f, cfg = step['term'], step['fused'], step['net'].cfg
    st = f['stats']
    assert {'loss', term + '_loss', 'img_loss', 'psnr', 'offset_loss', 'reg_dist'} <= set(st)
    other = cfg.reg_dist_weight * st['reg_dist'] + cfg.resd_loss_weight * st['offset_loss']
    if 'pair_loss' in st:
        other = other + cfg.pair_loss_weight * st['pair_loss']
    assert abs(float(f['loss']) - float(other + WEIGHT[term] * st[term + '_loss'] + st['img_loss'])) < 1e-6
    rgb, gt = f['ret']['rgb_map'].detach(), step['tb']['rgb']
    assert abs(float(st['img_loss']) - float(((rgb - gt) ** 2).mean())) < 1e-6
    assert abs(float(st['psnr']) - float(-10.0 * torch.log10(((rgb - gt) ** 2).mean()))) < 1e-3
    assert torch.allclose(f['error'], (rgb - gt).abs().sum(-1), atol=1e-6)
    p = step['plain']
    assert torch.allclose(rgb, p['ret']['rgb_map'].detach(), rtol=0, atol=1e-6)                  # the same render both times
    assert abs(float(f['loss']) - float(p['loss'])) < 1e-6


def statement(step, src):
    term, tb = step['term'], step['tb']
    H, W = int(tb['H'].item()), int(tb['W'].item())
    mask = tb['mask_at_box'][0].reshape(-1).cpu()
    rgb, gt = src['ret']['rgb_map'].detach()[0].cpu(), tb['rgb'][0].cpu()
    ip, ig = R.assemble(rgb, mask, H, W), R.assemble(gt, mask, H, W)
    if term == 'ssim':
        ex = R.ssim(ip, ig, R.gaussian_taps(11), np.float32(1.0), -WEIGHT[term])
        return R.E(1.0 - ex['ssim'].v, ex['ssim'].e + R.U), ex, mask
    occ = tb['occupancy'].reshape(-1).cpu().ne(0).to(torch.uint8)
    ex = R.tv(ip, ig, R.assemble(occ[:, None], mask, H, W)[0] != 0, np.float32(1.0), WEIGHT[term])
    return ex['tv'], ex, mask


def test_term_against_float64_and_the_op_by_op_path(step):
    term = step['term']
    for name in ('fused', 'plain'):
        value, _, _ = statement(step, step[name])
        got = step[name]['stats'][term + '_loss'].double().cpu()
        ok, ratio = value.holds(got)
        print('%s_loss %s %.9g  float64 %.9g  error / bound %.3f' % (term, name, float(got), float(value.v), ratio))
        assert ok, (name, ratio)


def test_fused_g_rgb_against_float64_and_the_op_by_op_path(step):
    f, p = step['fused'], step['plain']
    _, ex, mask = statement(step, f)
    n = float(f['g_rgb'].numel())
    rgb, gt = f['ret']['rgb_map'].detach()[0].cpu().double(), step['tb']['rgb'][0].cpu().double()
    mse = 2.0 * (rgb - gt) / n
    total = R.E(mse + R.rays(ex['gimg'].v, mask), R.rays(ex['gimg'].e, mask) + 4 * R.U * (mse.abs() + R.rays(ex['gimg'].v, mask).abs()))
    for name, src in (('fused', f), ('op-by-op', p)):
        ok, ratio = total.holds(src['g_rgb'][0].cpu())
        print('%s g_rgb %s error / bound %.3f (max |g| %.3g)' % (step['term'], name, ratio, float(src['g_rgb'].abs().max())))
        assert ok, (name, ratio)


def test_fused_g_rgb_reproduces_the_parameter_gradients(step):
    f, p = step['fused'], step['plain']
    assert torch.isfinite(f['g_rgb']).all() and float(f['g_rgb'].abs().max()) > 0
    checked = 0
    for name, a, b in zip(step['names'], f['grads'], p['grads']):
        assert (a is None) == (b is None), name
        if a is None:
            continue
        scale = max(float(b.abs().max()), 1e-6)
        assert float((a - b).abs().max()) <= 2e-4 * scale + 2e-7, (name, float((a - b).abs().max()), scale)
        checked += 1
    assert checked >= 20


def test_unrecognised_module_and_out_of_range_side_keep_the_op_by_op_path(step, monkeypatch):
    term, wrap, tb = step['term'], step['wrap'], step['tb']
    attr = 'ssim_loss' if term == 'ssim' else 'tv_image_loss'
    mod, seen = getattr(wrap, attr), []

    class Spy(torch.nn.Module):          # an injected stand-in no rule recognises
        def forward(self, *a):
            seen.append(a[0].shape)
            return mod(*a)
    gen = wrap._fused_image_terms.gen
    try:
        setattr(wrap, attr, Spy())
        _, loss_spy, stats_spy, _ = wrap(tb, split='train')
    finally:
        setattr(wrap, attr, mod)
    assert len(seen) == 1 and stats_spy[term + '_loss'].requires_grad and wrap._fused_image_terms.gen == gen
    monkeypatch.setattr(losses, 'IMGLOSS_MAX_SIDE', 32)                 # the 64 x 64 patch is out of range now
    _, loss_big, stats_big, _ = wrap(tb, split='train')
    assert stats_big[term + '_loss'].requires_grad and wrap._fused_image_terms.gen == gen
    monkeypatch.undo()
    _, loss_back, stats_back, _ = wrap(tb, split='train')
    assert not stats_back[term + '_loss'].requires_grad and wrap._fused_image_terms.gen == gen + 1
    for other in (loss_spy, loss_big, loss_back):
        assert abs(float(other.detach()) - float(step['fused']['loss'])) < 1e-6


def test_lpips_wins_over_ssim(small_setup):
    class ZeroLoss(torch.nn.Module):
        def forward(self, x, t):
            return (x * 0.0).sum()
    net, tb, pin = make(small_setup, builtin_image_terms=True, use_lpips=True, use_ssim=True, use_tv_image=True)
    wrap = pin(NetworkWrapper(net, perceptual_loss=ZeroLoss()))
    _, loss, stats, _ = wrap(tb, split='train')
    assert 'lpips_loss' in stats and 'ssim_loss' not in stats and 'tv_loss' not in stats
    net.cfg.use_lpips = False
    _, loss, stats, _ = wrap(tb, split='train')
    assert 'ssim_loss' in stats and 'tv_loss' not in stats and 'lpips_loss' not in stats          # then use_ssim, before use_tv_image
