"""GPU: the Evaluator's fourth metric on the device — invr.evaluator.Evaluator with an invr.lpips_eval.LpipsVgg (csrc/k_lpips.hip): the
value of every cfg.test_full frame equals the direct call bit for bit and the float64 checker within the end-to-end rule of
tests/test_gpu_lpips.py (8 noise), reaches metrics.npy and summarize(), and no evaluate() synchronises.  A module with the lpips
package's structure takes the device path, or with cfg.eval_fused_lpips False its own torch call (run here with MIOpen switched off
for the call, so that the suite does not pay its first-call search for 13 shapes; the two values are held to the same rule)."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import lpips_reference as R               # noqa: E402  (checker only)
from tests.test_gpu_lpips import perturbed           # noqa: E402

DEV = 'cuda:0'
FRAMES = ((24, 32), (37, 29), (16, 16))


def frame(k):
    """-> H, W, mask (H*W uint8, an ellipse), pred (n, 3), gt (n, 3): fp32 CPU tensors"""
    H, W = FRAMES[k]
    g = torch.Generator().manual_seed(4000 + k)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    mask = ((((yy - H / 2) / (0.45 * H)) ** 2 + ((xx - W / 2) / (0.4 * W)) ** 2) <= 1.0).reshape(-1).to(torch.uint8)
    n = int(mask.sum())
    pred = torch.rand(n, 3, generator=g)
    gt = (pred + torch.randn(n, 3, generator=g) * 0.05).clamp(0.0, 1.0)
    return H, W, mask, pred, gt


def images(k, dtype=torch.float32):
    H, W, mask, pred, gt = frame(k)
    out = []
    for v in (pred, gt):
        img = torch.zeros(H * W, 3, dtype=dtype)
        img[mask.bool()] = v.to(dtype)
        out.append(img.reshape(H, W, 3))
    return out


def batch_of(k):
    H, W, mask, pred, gt = frame(k)
    out = {'rgb_map': pred[None].to(DEV)}
    batch = {'mask_at_box': mask[None].to(DEV), 'rgb': gt[None].to(DEV), 'H': torch.tensor([H]), 'W': torch.tensor([W]),
             'frame_index': torch.tensor([k]), 'cam_ind': torch.tensor([0])}
    return out, batch


def oracle(k):
    """-> (float64 lpips, noise) of frame k by the rule of tests/test_gpu_lpips.py"""
    w = R.make_weights(0)
    p, t = images(k)
    f64 = float(R.forward(w, p, t)['lpips'])
    noise = abs(float(R.forward(w, p, t, torch.float32)['lpips']) - f64)
    g = torch.Generator().manual_seed(77)
    for _ in range(4):
        noise = max(noise, abs(float(R.forward(w, perturbed(p, g), perturbed(t, g))['lpips']) - f64))
    return f64, noise


def cfg_of(tmp_path, **kw):
    from invr.config import Node
    return Node(**dict(dict(test_full=True, fast_eval=True, dry_run=False, eval_part='', result_dir=str(tmp_path)), **kw))


def test_evaluator_lpips_equals_the_direct_calls_and_the_checker(tmp_path):
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    net = LpipsVgg.random(0)
    ev = Evaluator(cfg_of(tmp_path), lpips=net)
    direct = []
    for k in range(3):
        ev.evaluate(*batch_of(k))
        p, t = images(k)
        direct.append(net(p.to(DEV), t.to(DEV)))
    ev.collect()
    direct = [float(v) for v in torch.stack(direct).cpu()]
    assert ev.lpips == direct                                      # bit for bit: the same kernels on the same assembled images
    for k in range(3):
        f64, noise = oracle(k)
        print('evaluator lpips frame %d: %.9g   K %.3f' % (k, f64, abs(ev.lpips[k] - f64) / noise))
        assert abs(ev.lpips[k] - f64) <= 8.0 * noise, (k, ev.lpips[k], f64, noise)
    ret = ev.summarize()
    saved = np.load(os.path.join(str(tmp_path), 'metrics.npy'), allow_pickle=True).item()
    assert saved['lpips'] == direct and len(saved['mse']) == 3
    assert ret['lpips'] == np.mean(direct)
    assert ev.lpips == []


def test_recognised_module_takes_the_device_path_and_the_flag_keeps_it_on_torch(tmp_path):
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    w = R.make_weights(0)
    k = 2                                                          # the 16 x 16 frame
    f64, noise = oracle(k)
    p, t = images(k)
    direct = float(LpipsVgg.random(0)(p.to(DEV), t.to(DEV)).cpu())
    ev = Evaluator(cfg_of(tmp_path), lpips=R.Lpips(w))
    ev.evaluate(*batch_of(k))
    assert ev._lpips_fused is not None and ev._loss_fn is None
    ev.collect()
    assert ev.lpips == [direct]
    ev2 = Evaluator(cfg_of(tmp_path, eval_fused_lpips=False), lpips=R.Lpips(w))
    with torch.backends.cudnn.flags(enabled=False):
        ev2.evaluate(*batch_of(k))
    assert ev2._lpips_fused is None and isinstance(ev2._loss_fn, R.Lpips)
    ev2.collect()
    print('module paths: device %.9g torch %.9g float64 %.9g noise %.3g   K device %.3f torch %.3f between %.3f'
          % (direct, ev2.lpips[0], f64, noise, abs(direct - f64) / noise, abs(ev2.lpips[0] - f64) / noise, abs(ev2.lpips[0] - direct) / noise))
    assert abs(direct - f64) <= 8.0 * noise and abs(ev2.lpips[0] - f64) <= 8.0 * noise
    assert abs(ev2.lpips[0] - direct) <= 8.0 * noise
    # a module that is not recognised keeps its own call whatever the flag says
    class Other(torch.nn.Module):
        def forward(self, a, b):
            return ((a - b) ** 2).mean().reshape(1, 1, 1, 1)
    ev3 = Evaluator(cfg_of(tmp_path), lpips=Other())
    ev3.evaluate(*batch_of(k))
    assert ev3._lpips_fused is None and isinstance(ev3._loss_fn, Other)
    ev3.collect()
    assert abs(ev3.lpips[0] - float(((p - t) ** 2).mean())) <= 1e-6


def test_weights_from_the_configured_files(tmp_path):
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    from tests.test_lpips_loader_cpu import write_files
    pv, pl = write_files(tmp_path, R.make_weights(0))
    ev = Evaluator(cfg_of(tmp_path, lpips_vgg16_weights=pv, lpips_lin_weights=pl))
    ev.evaluate(*batch_of(2))
    ev.collect()
    p, t = images(2)
    assert ev.lpips == [float(LpipsVgg.random(0)(p.to(DEV), t.to(DEV)).cpu())]


def test_named_files_that_cannot_be_used_raise(tmp_path):
    from invr.evaluator import Evaluator
    from tests.test_lpips_loader_cpu import write_files
    pv, pl = write_files(tmp_path, R.make_weights(0), drop=('features.28.bias',))
    ev = Evaluator(cfg_of(tmp_path, lpips_vgg16_weights=pv, lpips_lin_weights=pl))
    with pytest.raises(KeyError, match='features.28.bias'):
        ev.evaluate(*batch_of(2))


def test_partial_frames_compute_nothing(tmp_path):
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    ev = Evaluator(cfg_of(tmp_path, test_full=False), lpips=LpipsVgg.random(0))
    ev.evaluate(*batch_of(0))
    assert ev._lpips_dev == [] and ev._lpips_state is None
    ret = ev.summarize()
    assert 'lpips' not in ret and np.load(os.path.join(str(tmp_path), 'metrics.npy'), allow_pickle=True).item()['lpips'] == []


def test_without_weights_the_list_stays_empty_and_the_warning_appears_once(tmp_path, monkeypatch):
    from invr.evaluator import Evaluator
    monkeypatch.setitem(sys.modules, 'lpips', None)                # `import lpips` raises ImportError, whatever this host has installed
    ev = Evaluator(cfg_of(tmp_path))
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        for k in range(3):
            ev.evaluate(*batch_of(k))
    assert len([r for r in rec if 'LPIPS is not computed' in str(r.message)]) == 1
    ev.collect()
    assert ev.lpips == [] and len(ev.mse) == 3
    assert 'lpips' not in ev.summarize()


def test_evaluate_issues_no_synchronisation(tmp_path):
    """Every evaluate() of the device path under torch.cuda.set_sync_debug_mode('error'), as the NoSync case of
    tests/test_gpu_eval_metrics.py; the last lines check that this runtime honours the mode."""
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    net = LpipsVgg.random(0)
    ev = Evaluator(cfg_of(tmp_path), lpips=net)
    work = [batch_of(k) for k in (0, 1, 2, 0)]                     # a grow and a reuse of the workspace
    torch.cuda.synchronize()
    for out, batch in work:
        torch.cuda.set_sync_debug_mode('error')
        try:
            ev.evaluate(out, batch)
        finally:
            torch.cuda.set_sync_debug_mode('default')
    ev.collect()
    assert len(ev.lpips) == 4 and ev.lpips[0] == ev.lpips[3]
    honoured = False
    torch.cuda.set_sync_debug_mode('error')
    try:
        torch.ones(1, device=DEV).sum().item()
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert honoured, 'set_sync_debug_mode is not honoured here: the no-synchronisation property was not checked'


def test_run_evaluate_device_returns_the_lpips_list():
    from invr import driver
    from invr.evaluator import Evaluator
    from invr.lpips_eval import LpipsVgg
    from tests.test_gpu_eval_metrics import _net, _sequence
    net = _net(dict(table_log2=12, N_samples=64))
    seq = _sequence(2, 48)
    lp = LpipsVgg.random(0)
    cfg = {'test_full': True, 'fast_eval': True, 'dry_run': False, 'eval_part': '', 'result_dir': ''}
    runs = [driver.run_evaluate(net, seq, device=DEV, in_flight=K, metrics='device', evaluator=Evaluator(cfg=dict(cfg), lpips=lp)) for K in (2, 1)]
    assert len(runs[0]['lpips']) == 2 and all(np.isfinite(v) and v > 0.0 for v in runs[0]['lpips'])
    assert runs[0]['lpips'] == runs[1]['lpips'] and runs[0]['mse'] == runs[1]['mse']
    plain = driver.run_evaluate(net, seq, device=DEV, in_flight=2, metrics='device')
    assert plain['mse'] == runs[0]['mse'] and ('lpips' not in plain or len(plain['lpips']) == 2)
