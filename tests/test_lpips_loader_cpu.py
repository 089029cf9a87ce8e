"""CPU: where invr.lpips_eval.LpipsVgg takes its weights from — tensors, a module with the lpips package's structure, the two files that
package loads — and what it refuses.  The tensor routes are compared value for value; the packed weight images of the three routes
are built on the CPU wave machine (tests/hostsim) and compared bit for bit."""
import pytest
import torch

from tests import lpips_reference as R
from invr import lpips_eval as E


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x.detach().reshape(-1), y.detach().reshape(-1)) for x, y in zip(a, b))


def write_files(tmp_path, weights, drop=()):
    conv_w, conv_b, lin_w = weights
    vgg = {}
    for l, i in enumerate(E.VGG16_CONVS):
        vgg['features.%d.weight' % i] = conv_w[l]
        vgg['features.%d.bias' % i] = conv_b[l]
    for k in ('classifier.0.weight', 'classifier.0.bias'):          # (a full state dict holds more than the features)
        vgg[k] = torch.zeros(2)
    lin = {'lin%d.model.1.weight' % k: lin_w[k].reshape(1, -1, 1, 1) for k in range(5)}
    for k in drop:
        vgg.pop(k, None)
        lin.pop(k, None)
    pv, pl = str(tmp_path / 'vgg16.pth'), str(tmp_path / 'vgg.pth')
    torch.save(vgg, pv)
    torch.save(lin, pl)
    return pv, pl


def test_random_is_the_checkers_rule():
    a, b = E.random_tensors(0), R.make_weights(0)
    assert all(same(x, y) for x, y in zip(a, b))
    assert all((t >= 0).all() for t in a[2])
    assert not same(E.random_tensors(1)[0], a[0])
    assert (tuple(E.CIN), tuple(E.COUT), tuple(E.TAPS), E.SHIFT, E.SCALE) == (R.CIN, R.COUT, R.TAPS, R.SHIFT, R.SCALE)


def test_module_and_files_round_trip(tmp_path):
    w = E.random_tensors(3)
    got = E.module_tensors(R.Lpips(w))
    assert got is not None
    assert same(got[0], w[0]) and same(got[1], w[1]) and same(got[2], w[2])
    assert torch.equal(got[3], torch.tensor(E.SHIFT)) and torch.equal(got[4], torch.tensor(E.SCALE))
    f = E.file_tensors(*write_files(tmp_path, w))
    assert same(f[0], w[0]) and same(f[1], w[1]) and same(f[2], w[2])


def test_other_modules_are_not_recognised():
    w = E.random_tensors(3)
    assert E.module_tensors(R.Lpips(w)) is not None
    cout = list(R.COUT)
    cin = list(R.CIN)
    cout[4], cin[5] = 128, 128                               # a wrong channel plan
    assert E.module_tensors(R.Lpips(None, tuple(cin), tuple(cout))) is None
    assert E.module_tensors(R.Lpips(w, lin_bias=True)) is None          # a biased lin
    assert E.module_tensors(R.Lpips(w, scaling=False)) is None          # no scaling layer
    m = R.Lpips(w)
    m.net.slice1.conv0.padding = (0, 0)
    assert E.module_tensors(m) is None
    m = R.Lpips(w)
    m.net.slice5.add_module('extra', torch.nn.Conv2d(512, 512, 3, padding=1))
    assert E.module_tensors(m) is None
    m = R.Lpips(w)
    del m.lin4
    assert E.module_tensors(m) is None
    assert E.module_tensors(torch.nn.Linear(3, 3)) is None and E.LpipsVgg.from_module(torch.nn.Linear(3, 3)) is None


def test_missing_keys_raise_and_list_what_was_found(tmp_path):
    w = E.random_tensors(3)
    with pytest.raises(KeyError) as e:
        E.file_tensors(*write_files(tmp_path, w, drop=('features.28.bias',)))
    assert "missing ['features.28.bias']" in str(e.value) and 'features.28.weight' in str(e.value) and 'classifier.0.weight' in str(e.value)
    with pytest.raises(KeyError) as e:
        E.file_tensors(*write_files(tmp_path, w, drop=('lin2.model.1.weight',)))
    assert 'lin2.model.1.weight' in str(e.value) and 'lin3.model.1.weight' in str(e.value) and 'vgg.pth' in str(e.value)


def test_wrong_shapes_raise():
    cw, cb, lw = E.random_tensors(3)
    with pytest.raises(ValueError, match='13 convolution weights'):
        E.LpipsVgg.from_tensors(cw[:12], cb, lw, device='cpu')
    with pytest.raises(ValueError, match='convolution 1 has weight'):
        E.LpipsVgg.from_tensors([cw[0], cw[0]] + cw[2:], cb, lw, device='cpu')
    with pytest.raises(ValueError, match='lin4 has 3 weights'):
        E.LpipsVgg.from_tensors(cw, cb, lw[:4] + [torch.zeros(3)], device='cpu')
    net = E.LpipsVgg(torch.zeros(4))                         # images elsewhere than the weights are refused ahead of the library
    with pytest.raises(ValueError, match='the weights are on cpu, the images on meta'):
        net(torch.zeros(16, 16, 3, device='meta'), torch.zeros(16, 16, 3, device='meta'))
    with pytest.raises(ValueError, match=r'two \(H,W,3\) images'):
        net(torch.zeros(16, 16), torch.zeros(16, 16))


def test_the_three_routes_pack_the_same_image(tmp_path):
    from tests.hostsim import harness
    w = E.random_tensors(3)
    with harness.activate():
        a = E.LpipsVgg.from_tensors(*w, device='cpu').packed
        b = E.LpipsVgg.from_module(R.Lpips(w), device='cpu').packed
        c = E.LpipsVgg.from_files(*write_files(tmp_path, w), device='cpu').packed
        from invr import _abi
        assert a.numel() == _abi.lib().invr_lpips_packed_floats()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    # the tail of the image: the 13 biases, the five lin vectors, shift and scale
    tail = torch.cat(list(w[1]) + list(w[2]) + [torch.tensor(E.SHIFT), torch.tensor(E.SCALE)])
    assert torch.equal(a[-tail.numel():], tail)
