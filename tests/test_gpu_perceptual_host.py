"""GPU: the host layer of the HIP perceptual loss — autograd.TrainLossPerceptualFn, losses.FusedPerceptual and NetworkWrapper with
cfg.use_lpips on the golden 64 x 64 scene.

  * loss == regulariser terms + lpips_loss (no separate MSE term), lpips_loss within 8 noise of the float64 loss of the same
    rgb_map (noise: the op-by-op path's own deviation and four ulp-sized perturbations, tests/test_gpu_perceptual.py);
  * parameter gradients through the layer-local statement only: the fused g_rgb fed into the op-by-op graph reproduces the fused
    path's parameter gradients (the two paths' g_rgb are NOT compared element-wise: independent ReLU / sign / pool decisions);
  * an unrecognised perceptual module keeps the op-by-op path; the packed weights follow an in-place weight change.
tests/test_hostsim_perceptual_cpu.py runs the same bodies on the CPU wave machine under HOSTSIM_FULL=1."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import perceptual_reference as R          # noqa: E402  (checker only)
from invr.network import Network                     # noqa: E402
from invr.trainer import NetworkWrapper, assemble_patch     # noqa: E402
from invr.losses import PerceptualLoss, FusedPerceptual, vgg_convs     # noqa: E402

DEV = 'cuda:0'


def seeded_loss(seed=3):
    """PerceptualLoss with the checker's seeded N(0, 2 / fan_in) weights (random ImageNet-free features: the kernels are weight-agnostic)."""
    pl = PerceptualLoss(allow_random=True)
    ws, bs = R.make_weights(seed)
    with torch.no_grad():
        for c, w, b in zip(vgg_convs(pl), ws, bs):
            c.weight.copy_(w)
            c.bias.copy_(b)
    return pl


class ZeroLoss(torch.nn.Module):
    """An injected stand-in no rule recognises: the op-by-op path, with an image term of exactly 0 and an exactly-zero gradient."""
    calls = 0

    def forward(self, x, t):
        self.calls += 1
        return (x * 0.0).sum()


@pytest.fixture(scope='module')
def step(small_setup):
    """One training iteration of NetworkWrapper with use_lpips on the HIP path, then the same iteration on the op-by-op graph with a
    zero image term and the fused g_rgb fed into rgb_map."""
    cfg, sd, batch, _ = small_setup
    net = Network(cfg=copy.deepcopy(cfg))
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).train()
    net.cfg.use_lpips = True
    gb = {k: v.to(DEV) for k, v in batch.items()}
    n, S = gb['ray_o'].shape[1], net.cfg.N_samples
    g = torch.Generator().manual_seed(5)
    jitter, noise = torch.rand(n, S, generator=g), torch.rand(n * S * 5, 3, generator=g)
    pl = seeded_loss()
    wrap = NetworkWrapper(net, perceptual_loss=pl)
    wrap.renderer._jitter = lambda shape, device: jitter.to(device)
    wrap.renderer._pair_noise_dense = lambda rows, device: noise.to(device)[:rows]
    tb = dict(gb)
    tb['iter_step'] = 2
    params = [p for p in net.parameters() if p.requires_grad]

    def grads():
        out = [None if p.grad is None else p.grad.detach().clone() for p in params]
        for p in params:
            p.grad = None
        return out
    ret, loss, stats, _ = wrap(tb, split='train')
    ret['rgb_map'].retain_grad()
    loss.backward()
    fused = {'ret': ret, 'loss': loss.detach(), 'stats': {k: v.detach() for k, v in stats.items()}, 'g_rgb': ret['rgb_map'].grad.clone(),
             'grads': grads(), 'error': ret['error'].detach().clone()}
    zero = ZeroLoss()
    wrap.perceptual_loss = zero
    ret2, loss2, stats2, _ = wrap(tb, split='train')
    torch.autograd.backward([ret2['rgb_map'], loss2], [fused['g_rgb'], torch.ones_like(loss2)])
    plain = {'ret': ret2, 'loss': loss2.detach(), 'stats': stats2, 'grads': grads(), 'calls': zero.calls}
    wrap.perceptual_loss = pl
    return {'wrap': wrap, 'net': net, 'pl': pl, 'tb': tb, 'fused': fused, 'plain': plain, 'names': [k for k, p in net.named_parameters() if p.requires_grad]}


def test_loss_is_regularisers_plus_lpips(step):
    f, cfg = step['fused'], step['net'].cfg
    st = f['stats']
    assert {'loss', 'lpips_loss', 'img_loss', 'psnr', 'offset_loss', 'reg_dist'} <= set(st)
    other = cfg.reg_dist_weight * st['reg_dist'] + cfg.resd_loss_weight * st['offset_loss']
    if 'pair_loss' in st:
        other = other + cfg.pair_loss_weight * st['pair_loss']
    assert abs(float(f['loss']) - float(other + st['lpips_loss'])) < 1e-6            # no separate MSE term (inb_trainer.py:206-209)
    # the statistics and ret['error'] as on the op-by-op path
    rgb, gt = f['ret']['rgb_map'].detach(), step['tb']['rgb']
    assert abs(float(st['img_loss']) - float(((rgb - gt) ** 2).mean())) < 1e-6
    assert abs(float(st['psnr']) - float(-10.0 * torch.log10(((rgb - gt) ** 2).mean()))) < 1e-3
    assert torch.allclose(f['error'], (rgb - gt).abs().sum(-1), atol=1e-6)
    assert torch.allclose(f['ret']['rgb_map'].detach(), step['plain']['ret']['rgb_map'].detach(), rtol=0, atol=1e-6)          # the same render both times
    assert abs(float(step['plain']['loss']) - float(other)) < 1e-6 and step['plain']['calls'] == 1      # the stand-in ran op-by-op


def test_lpips_value_against_float64_and_the_op_by_op_path(step):
    f, pl, tb = step['fused'], step['pl'], step['tb']
    H, W = int(tb['H'].item()), int(tb['W'].item())
    rgb, gt = f['ret']['rgb_map'].detach()[0], tb['rgb'][0]
    with torch.no_grad():
        ip, ig = assemble_patch(rgb, tb['mask_at_box'][0], H, W), assemble_patch(gt, tb['mask_at_box'][0], H, W)
        op_by_op = pl(ip.permute(2, 0, 1)[None], ig.permute(2, 0, 1)[None]).double().cpu()          # the parent commit's path
    ws, bs = R.make_weights(3)
    mask = tb['mask_at_box'][0].reshape(-1).cpu()
    img = lambda v: R.assemble(v, mask, H, W)
    exact = R.forward(ws, bs, img(rgb.cpu().double()), img(gt.cpu().double()))['loss']
    noise = max(float((op_by_op - exact).abs()), float((R.forward(ws, bs, img(rgb.cpu()), img(gt.cpu()), torch.float32)['loss'].double() - exact).abs()))
    g = torch.Generator().manual_seed(77)
    from tests.test_gpu_perceptual import perturbed
    for _ in range(4):
        noise = max(noise, float((R.forward(ws, bs, img(perturbed(rgb.cpu(), g)), img(perturbed(gt.cpu(), g)))['loss'] - exact).abs()))
    got = float(f['stats']['lpips_loss'].double().cpu())
    print('lpips fused %.9g  op-by-op %.9g  float64 %.9g  noise %.3g' % (got, float(op_by_op), float(exact), noise))
    assert abs(got - float(exact)) <= 8.0 * noise
    assert abs(float(op_by_op) - float(exact)) <= 8.0 * noise


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


def test_switch_and_unrecognised_modules_keep_the_op_by_op_path(step):
    wrap, tb = step['wrap'], step['tb']
    seen = []

    class Spy(torch.nn.Module):
        def forward(self, x, t):
            seen.append(x.shape)
            return step['pl'](x, t)
    assert vgg_convs(Spy()) is None and vgg_convs(step['pl']) is not None
    pl = wrap.perceptual_loss
    try:
        wrap.perceptual_loss = Spy()
        _, loss_spy, stats_spy, _ = wrap(tb, split='train')
        assert len(seen) == 1 and seen[0][1] == 3
        wrap.perceptual_loss = pl
        wrap.cfg.fused_perceptual = False                 # the A/B switch: the recognised module through torch ops
        gen = wrap._fused_perceptual.gen
        _, loss_off, stats_off, _ = wrap(tb, split='train')
        assert wrap._fused_perceptual.gen == gen and stats_off['lpips_loss'].requires_grad
    finally:
        wrap.perceptual_loss = pl
        wrap.cfg.fused_perceptual = True
    assert abs(float(loss_spy.detach()) - float(loss_off.detach())) < 1e-6
    assert abs(float(stats_off['lpips_loss']) - float(step['fused']['stats']['lpips_loss'])) < 1e-5


def test_packed_weights_follow_an_in_place_change():
    pl = seeded_loss().to(DEV)
    fp = FusedPerceptual()
    convs = vgg_convs(pl)
    a = fp.packed(convs)
    assert fp.packed(convs) is a                          # cached
    before = a.clone()
    with torch.no_grad():
        convs[1].weight.mul_(2.0)
    b = fp.packed(convs)
    assert not torch.equal(b, before)
    fresh = FusedPerceptual().packed(convs)
    assert torch.equal(b, fresh)
    assert vgg_convs(torch.nn.Linear(2, 2)) is None
