"""CPU: the checker of the perceptual-loss tests (tests/perceptual_reference.py) pinned against float64 autograd of
invr.losses.PerceptualLoss.double(): the loss to 16 n 2^-53 A, and — with the decisions taken from that same float64 run — the
gradient to the same bound (A: the absolute-value companion, n: the summand count)."""
import pytest
import torch

from invr.losses import PerceptualLoss, vgg_convs
from tests import perceptual_reference as R

CASES = ((2, 2, 0.05), (3, 3, 0.002), (9, 7, 0.05), (17, 15, 0.002), (33, 16, 0.05), (24, 40, 0.002))


def module64(ws, bs):
    pl = PerceptualLoss(allow_random=True).double()
    with torch.no_grad():
        for c, w, b in zip(vgg_convs(pl), ws, bs):
            c.weight.copy_(w)
            c.bias.copy_(b)
    return pl


@pytest.mark.parametrize('H,W,sigma', CASES)
def test_checker_against_float64_autograd(H, W, sigma):
    g = torch.Generator().manual_seed(H * 100 + W)
    ws, bs = R.make_weights(1)
    mask = (torch.rand(H * W, generator=g) < 0.8).to(torch.uint8)
    mask[0] = 1
    n = int(mask.sum())
    rgb = torch.rand(n, 3, generator=g).double()
    gt = (rgb + torch.randn(n, 3, generator=g).double() * sigma).clamp(0.0, 1.0)
    pl = module64(ws, bs)
    x = R.assemble(rgb, mask, H, W).requires_grad_()
    t = R.assemble(gt, mask, H, W)
    loss = pl(x[None], t[None])
    loss.backward()
    f = R.forward(ws, bs, x.detach(), t)
    u = 16 * 2.0 ** -53
    assert abs(float(f['loss'] - loss.detach())) <= u * f['c'] * float(f['A'])
    b = R.backward(ws, x.detach(), t, R.Decisions.of(f), 1.0)
    assert ((b['gimg'] - x.grad).abs() <= u * b['c'] * b['A']).all(), float(((b['gimg'] - x.grad).abs() / (b['A'] + 1e-300)).max())
    assert float(b['A'].min()) >= 0 and float(x.grad.abs().max()) > 0
    # the fp32 mode is the same arithmetic in fp32: close to, and not identical with, the float64 one
    f32 = R.forward(ws, bs, x.detach().float(), t.float(), torch.float32)
    assert f32['loss'].dtype == torch.float32 and abs(float(f32['loss'].double() - f['loss'])) <= 1e-5 * float(f['loss'])


def test_pool_rules():
    a = torch.tensor([[[1.0, 1.0, 5.0], [1.0, 0.0, 7.0], [9.0, 9.0, 9.0]]])          # 3 x 3: the last row / column feeds no pooled unit
    assert R.pool(a).tolist() == [[[1.0]]] and R.pool_first(a).tolist() == [[[0]]]     # the FIRST maximum of a tie
    assert R.pool_route(torch.tensor([[[2.0]]]), R.pool_first(a), 3, 3).tolist() == [[[2.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]]
    b = torch.tensor([[[0.0, 3.0], [3.0, 3.0]]])
    assert R.pool_first(b).tolist() == [[[1]]]
