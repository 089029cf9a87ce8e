"""GPU: the on-device evaluation metrics (invr.metrics / invr.evaluator over csrc/k_metrics.hip) against the float64 NumPy restatement of
the reference's Evaluator in tests/eval_metrics_reference.py — never against the code under test.  The bodies run on DEV;
tests/test_hostsim_eval_metrics_cpu.py borrows them for the wave machine (DEV = 'cpu' under harness.activate()).

Bounds (each against the restatement): assembled images, rectangle, window count, status, uint8 images: exact (copies and integer
results; float32 x 255 is exact in float64, so the rounded byte is defined bit for bit).  SSE and sum gt: relative 1e-9 — every term is
exact up to one rounding and a sum of N <= 3 * 1024^2 non-negative float64 terms in any order is within N * 2^-53 = 3.5e-10 of the true
sum.  SSIM: absolute 1e-9 — window means of 49 float64 terms carry <= 5.4e-15 absolute error, the factor vx + vy + C2 >= 3.6e-3 bounds
the relative error of S near 3e-11 and |S| <= 1.  psnr: absolute 4.35e-9 (= 10 / ln 10 x the 1e-9 on mse).

Not exercised anywhere here: a comparison with scikit-image / OpenCV themselves (neither is installed in this project's environment; the
skimage branch below runs only where the package happens to be importable, the uint8 rounding rule is OpenCV's documented one)."""
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

from tests import eval_metrics_reference as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'

SMALL = [(16, 16), (64, 48), (97, 131)]
MASKS = ['full', 'ellipse', 'borders', 'single', 'empty', 'strip']
CONTENTS = ['noise', 'equal', 'bright']


def make_mask(kind, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == 'full':
        m = np.ones((H, W), bool)
    elif kind == 'ellipse':
        m = ((yy - 0.55 * H) / (0.33 * H)) ** 2 + ((xx - 0.45 * W) / (0.27 * W)) ** 2 <= 1.0
    elif kind == 'borders':                    # an ellipse wider than the frame: touches all four borders, corners unset
        m = ((yy - (H - 1) / 2) / (0.56 * H)) ** 2 + ((xx - (W - 1) / 2) / (0.56 * W)) ** 2 <= 1.0
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any() and not m[0, 0]
    elif kind == 'single':
        m = np.zeros((H, W), bool)
        m[H // 3, (2 * W) // 3] = True
    elif kind == 'empty':
        m = np.zeros((H, W), bool)
    elif kind == 'strip':                      # 5 pixels wide: no 7x7 window inside its rectangle
        m = np.zeros((H, W), bool)
        m[2:H - 1, W // 2:W // 2 + 5] = True
    else:
        raise KeyError(kind)
    return m.reshape(-1)


def make_values(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        gt = rng.random((n, 3), dtype=np.float32)
        pred = rng.random((n, 3), dtype=np.float32)
    elif kind == 'equal':
        gt = rng.random((n, 3), dtype=np.float32)
        pred = gt.copy()
    elif kind == 'bright':                     # smooth and bright: uxx - ux^2 cancels to ~1e-6 of its terms
        base = np.linspace(0.85, 0.95, max(n, 1), dtype=np.float64)[:n, None] * np.ones((1, 3))
        gt = (base + 1e-3 * rng.standard_normal((n, 3))).astype(np.float32)
        pred = (base + 1e-3 * rng.standard_normal((n, 3))).astype(np.float32)
    else:
        raise KeyError(kind)
    return pred, gt


def run_kernels(pred, gt, mask, H, W, crop, want_u8=True, n_rows=None):
    from invr import metrics as M
    dev = torch.device(DEV)
    res = M.new_results(1, dev)
    ws = M.new_workspace(H, W, dev)
    ws.fill_(0xA5)                              # nothing may read what it has not written
    tp = torch.from_numpy(pred if n_rows is None else pred[:n_rows]).to(dev)
    tg = torch.from_numpy(gt if n_rows is None else gt[:n_rows]).to(dev)
    tm = torch.from_numpy(mask).to(dev)
    imgs = M.image_assemble(tp, tg, tm, H, W, res[0], ws, want_u8=want_u8)
    M.image_metrics(imgs[0], imgs[1], res[0], ws, crop=crop)
    if dev.type == 'cuda':
        torch.cuda.synchronize()
    return M.decode(res[0].cpu()), [None if t is None else t.cpu().numpy() for t in imgs]


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


def check_frame(H, W, mask_kind, content, test_full, seed=0):
    mask = make_mask(mask_kind, H, W)
    n = int(mask.sum())
    pred, gt = make_values(content, n, seed + 17 * H + W)
    want = R.frame_metrics(pred, gt, mask, H, W, test_full=test_full)
    got, (img_p, img_g, u8_p, u8_g) = run_kernels(pred, gt, mask, H, W, crop=not test_full)
    assert img_p.dtype == np.float32 and np.array_equal(img_p, want['img_pred']) and np.array_equal(img_g, want['img_gt'])
    assert np.array_equal(u8_p, want['u8_pred']) and np.array_equal(u8_g, want['u8_gt'])
    assert (got['x'], got['y'], got['w'], got['h']) == want['rect']
    assert got['status'] == 0 and got['n_set'] == n
    assert got['windows'] == want['windows']
    print('%dx%d %s %s full=%d: sse %.17g (ref %.17g, rel %.2e)  sum_gt rel %.2e' % (
        H, W, mask_kind, content, test_full, got['sse'], want['sse'], rel(got['sse'], want['sse']) if want['sse'] else 0.0,
        rel(got['sum_gt'], want['sum_gt']) if want['sum_gt'] else 0.0))
    if content == 'equal' or n == 0:
        assert got['sse'] == 0.0
    else:
        assert rel(got['sse'], want['sse']) <= 1e-9
    if n == 0:
        assert got['sum_gt'] == 0.0
    else:
        assert rel(got['sum_gt'], want['sum_gt']) <= 1e-9
    from invr import metrics as M
    if want['windows'] == 0:
        with pytest.raises(ValueError):
            M.ssim_of(got)
        return
    ssim = M.ssim_of(got)
    print('    ssim %.17g (ref %.17g, abs %.2e)' % (ssim, want['ssim'], abs(ssim - want['ssim'])))
    assert abs(ssim - want['ssim']) <= 1e-9
    if content == 'equal':
        assert abs(ssim - 1.0) <= 1e-12
    if n:
        mse = M.mse_of(got, H, W, test_full)
        assert rel(mse, want['mse']) <= 1e-9 if want['mse'] else mse == 0.0


@pytest.mark.parametrize('test_full', [True, False], ids=['full', 'crop'])
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('mask_kind', MASKS)
@pytest.mark.parametrize('size', SMALL, ids=lambda s: '%dx%d' % s)
def test_metrics_kernels(size, mask_kind, content, test_full):
    check_frame(size[0], size[1], mask_kind, content, test_full)


@pytest.mark.parametrize('test_full', [True, False], ids=['full', 'crop'])
@pytest.mark.parametrize('content', CONTENTS)
@pytest.mark.parametrize('mask_kind', MASKS)
def test_metrics_kernels_512(mask_kind, content, test_full):
    check_frame(512, 512, mask_kind, content, test_full)


def test_mask_row_count_mismatch_sets_status_and_stays_in_bounds():
    H, W = 64, 48
    mask = make_mask('ellipse', H, W)
    n = int(mask.sum())
    pred, gt = make_values('noise', n, 3)
    for rows in (n - 5, n - 1):                  # fewer rows than set pixels: the surplus pixels stay zero, nothing past the rows is read
        got, (img_p, img_g, _, _) = run_kernels(pred, gt, mask, H, W, crop=False, n_rows=rows)
        assert got['status'] != 0 and got['n_set'] == n
        want = np.zeros((H * W, 3), np.float32)
        want[np.nonzero(mask)[0][:rows]] = pred[:rows]
        assert np.array_equal(img_p.reshape(-1, 3), want)
    extra = np.concatenate([pred, pred[:4]]), np.concatenate([gt, gt[:4]])
    got, _ = run_kernels(extra[0], extra[1], mask, H, W, crop=False)          # more rows than set pixels
    assert got['status'] != 0


def test_argument_errors_do_not_touch_the_device():
    from invr import _abi, metrics as M
    L = _abi.lib()
    assert L.invr_eval_workspace_bytes(-1, 4) == 0
    assert 0 < L.invr_eval_workspace_bytes(16, 16) < L.invr_eval_workspace_bytes(512, 512)
    assert L.invr_image_metrics(None, None, 8, 8, 0, None, None, 0, None) != 0 and b'null' in L.invr_last_error()
    assert L.invr_image_assemble(None, None, None, 3, 8, 8, None, None, None, None, None, None, 0, None) != 0
    dev = torch.device(DEV)
    res, ws = M.new_results(1, dev), M.new_workspace(8, 8, dev)
    img = torch.zeros((128, 128, 3), device=dev)
    with pytest.raises(RuntimeError, match='workspace too small'):
        M.image_metrics(img, img, res[0], ws)
    with pytest.raises(ValueError):
        M.image_assemble(torch.zeros((3, 3), device=dev), torch.zeros((3, 3), device=dev), torch.ones(10, dtype=torch.bool, device=dev), 4, 4, res[0], ws)


def test_results_are_bit_identical_run_to_run():
    H, W = 97, 131
    mask = make_mask('ellipse', H, W)
    pred, gt = make_values('noise', int(mask.sum()), 11)
    runs = [run_kernels(pred, gt, mask, H, W, crop=c)[0] for c in (False, False, True, True)]
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert np.float64(a['sse']).tobytes() == np.float64(b['sse']).tobytes()
        assert np.float64(a['sum_s']).tobytes() == np.float64(b['sum_s']).tobytes()


# ---- Evaluator ----------------------------------------------------------------------------------------------------------------------
def make_batch(mask, gt, H, W, frame, cam, dev):
    return {'mask_at_box': torch.from_numpy(mask.reshape(1, -1)).to(dev), 'rgb': torch.from_numpy(gt[None]).to(dev),
            'H': torch.tensor([H]), 'W': torch.tensor([W]), 'frame_index': torch.tensor([frame]), 'cam_ind': torch.tensor([cam])}


def evaluator_frames():
    frames = []
    for k, (size, mk, content) in enumerate([((64, 48), 'ellipse', 'noise'), ((97, 131), 'borders', 'bright'), ((16, 16), 'full', 'noise'),
                                              ((64, 48), 'empty', 'noise'), ((97, 131), 'ellipse', 'equal')]):
        mask = make_mask(mk, *size)
        pred, gt = make_values(content, int(mask.sum()), 100 + k)
        if content == 'equal':
            pred = (gt * np.float32(0.5)).astype(np.float32)          # (mse 0 has no psnr)
        frames.append((size, mask, pred, gt))
    return frames


@pytest.mark.parametrize('test_full', [True, False], ids=['full', 'crop'])
def test_evaluator_matches_restatement(tmp_path, test_full):
    from invr.config import Node
    from invr.evaluator import Evaluator
    dev = torch.device(DEV)
    cfg = Node(test_full=test_full, fast_eval=True, dry_run=False, eval_part='', result_dir=str(tmp_path))
    ev = Evaluator(cfg=cfg)
    want = {'mse': [], 'psnr': [], 'ssim': []}
    for k, ((H, W), mask, pred, gt) in enumerate(evaluator_frames()):
        out = {'rgb_map': torch.from_numpy(pred[None]).to(dev if k % 2 == 0 else 'cpu')}          # device tensors and host tensors
        assert ev.evaluate(out, make_batch(mask, gt, H, W, k, 0, dev)) is None
        ref = R.frame_metrics(pred, gt, mask, H, W, test_full=test_full)
        if not test_full and ref['sum_gt'] == 0:
            continue                                                                              # if_nerf.py:134-135
        for key in ('mse', 'ssim'):
            want[key].append(ref[key])
        with np.errstate(divide='ignore'):
            want['psnr'].append(R.psnr(ref['mse']))
    ret = ev.summarize()
    saved = np.load(os.path.join(str(tmp_path), 'metrics.npy'), allow_pickle=True).item()
    assert set(saved) == {'mse', 'psnr', 'ssim', 'lpips'} and set(ret) >= {'psnr', 'ssim'}
    assert len(saved['mse']) == len(want['mse']) == (5 if test_full else 4)
    for got, ref in zip(saved['mse'], want['mse']):
        assert got == ref == 0.0 or rel(got, ref) <= 1e-9
    for got, ref in zip(saved['psnr'], want['psnr']):
        assert (np.isinf(got) and np.isinf(ref)) or abs(got - ref) <= 4.35e-9
    for got, ref in zip(saved['ssim'], want['ssim']):
        assert abs(got - ref) <= 1e-9
    with np.errstate(invalid='ignore'):
        assert abs(ret['ssim'] - np.mean(want['ssim'])) <= 1e-9
        finite = np.isfinite(want['psnr']).all()
        assert not finite or abs(ret['psnr'] - np.mean(want['psnr'])) <= 4.35e-9
    assert ev.mse == [] and ev.psnr == [] and ev.ssim == [] and ev.lpips == []             # (:175-178)
    # epoch-numbered file, and results() before summarize()
    (H, W), mask, pred, gt = evaluator_frames()[0]
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt, H, W, 0, 0, dev), epoch=3)
    r = ev.results()
    assert len(r) == 1 and r[0]['status'] == 0 and r[0]['n_set'] == int(mask.sum())
    ev.summarize(epoch=3)
    assert os.path.exists(os.path.join(str(tmp_path), 'metrics_epoch3.npy'))


def test_evaluator_no_window_frame_raises_and_mismatch_raises(tmp_path):
    from invr.config import Node
    from invr.evaluator import Evaluator
    dev = torch.device(DEV)
    H, W = 64, 48
    ev = Evaluator(cfg=Node(test_full=False, fast_eval=True, dry_run=False, eval_part='', result_dir=str(tmp_path)))
    mask = make_mask('strip', H, W)
    pred, gt = make_values('noise', int(mask.sum()), 1)
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt, H, W, 0, 0, dev))
    with pytest.raises(ValueError):
        ev.summarize()
    ev = Evaluator(cfg=Node(test_full=True, fast_eval=True, dry_run=False, eval_part='', result_dir=str(tmp_path)))
    mask = make_mask('ellipse', H, W)
    pred, gt = make_values('noise', int(mask.sum()) - 2, 1)
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt, H, W, 0, 0, dev))
    with pytest.raises(RuntimeError, match='mask'):
        ev.summarize()
    with pytest.raises(ValueError, match='eval_part'):
        Evaluator(cfg=Node(test_full=True, fast_eval=True, dry_run=False, eval_part='head', result_dir=str(tmp_path)))
    ev = Evaluator(cfg=Node(test_full=True, fast_eval=True, dry_run=True, eval_part='', result_dir=str(tmp_path)))
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt[:len(pred)], H, W, 0, 0, dev))
    assert ev.summarize() is None and ev.results() == []                                    # dry_run (:109-110, :150-151)


def test_evaluator_writes_the_reference_png_names(tmp_path):
    """fast_eval off: frame{:04d}_view{:04d}(_gt).png under comparison/ (comparison_epoch{N}/), holding the uint8 device image."""
    from invr.config import Node
    from invr import evaluator as E
    if E.image_writer() is None:
        with pytest.raises(RuntimeError, match='cv2'):
            E.write_png(str(tmp_path / 'x.png'), np.zeros((4, 4, 3), np.uint8))
        return
    dev = torch.device(DEV)
    H, W = 64, 48
    mask = make_mask('ellipse', H, W)
    pred, gt = make_values('noise', int(mask.sum()), 2)
    ev = E.Evaluator(cfg=Node(test_full=True, fast_eval=False, dry_run=False, eval_part='', result_dir=str(tmp_path)))
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt, H, W, 7, 2, dev), epoch=4)
    ev.evaluate({'rgb_map': torch.from_numpy(pred[None]).to(dev)}, make_batch(mask, gt, H, W, 7, 2, dev))
    ev.summarize()
    from PIL import Image
    want = R.frame_metrics(pred, gt, mask, H, W)
    for d in ('comparison_epoch4', 'comparison'):
        for name, key in (('frame0007_view0002.png', 'u8_pred'), ('frame0007_view0002_gt.png', 'u8_gt')):
            got = np.asarray(Image.open(os.path.join(str(tmp_path), d, name)))                  # (PIL reads R,G,B)
            assert np.array_equal(got[..., ::-1], want[key])


def test_plugin_evaluator_resolves_with_the_reference_signatures():
    """`evaluator_module invr.plugin.evaluator` (lib/evaluators/make_evaluator.py:5-8 imports the module and calls .Evaluator())."""
    import invr  # noqa: F401
    mod = importlib.import_module('invr.plugin.evaluator')

    class Stub:                                    # the reference's parameter names (if_nerf.py:76, :146)
        def evaluate(self, output, batch, epoch=-1): pass
        def summarize(self, epoch=-1): pass
    for name in ('evaluate', 'summarize'):
        assert inspect.signature(getattr(mod.Evaluator, name)) == inspect.signature(getattr(Stub, name))
    ev = mod.Evaluator()
    assert (ev.mse, ev.psnr, ev.ssim, ev.lpips) == ([], [], [], [])


# ---- driver.run_evaluate(metrics='device'): GPU only ------------------------------------------------------------------------------
def _net(cfg_kw, sd=None):
    import invr  # noqa: F401
    from invr import params
    from invr.config import make_cfg
    from invr.network import Network
    cfg = make_cfg(**cfg_kw) if isinstance(cfg_kw, dict) else cfg_kw
    net = Network(cfg=cfg)
    net.load_state_dict(sd if sd is not None else params.init_state_dict(cfg, seed=4), strict=True)
    return net.to('cuda:0').eval()


def _sequence(n, res):
    from invr import scene
    out = []
    for k in range(n):
        b, _ = scene.make_scene(res, res, seed=0, cam_dist=1.8, frame=(3 + 7 * k) % 100, pose_seed=k)
        out.append(scene.to_torch(b))
    return out


def gpu_only(fn):
    fn.gpu_only = True
    return fn


@gpu_only
def test_run_evaluate_device_equals_host_on_the_golden_scene(small_setup):
    from invr import driver
    cfg, sd, batch, _ = small_setup
    net = _net(cfg, sd)
    host = driver.run_evaluate(net, [batch], device='cuda:0', in_flight=1)
    dev = driver.run_evaluate(net, [batch], device='cuda:0', in_flight=1, metrics='device')
    assert set(dev) >= {'mse', 'psnr', 'ssim'} and len(dev['mse']) == len(dev['ssim']) == 1
    print('golden scene: mse host %.17g device %.17g' % (host['mse'][0], dev['mse'][0]))
    assert rel(dev['mse'][0], host['mse'][0]) <= 1e-9 and abs(dev['psnr'][0] - host['psnr'][0]) <= 4.35e-9
    assert 0.0 < dev['ssim'][0] <= 1.0


@gpu_only
def test_run_evaluate_device_sequence_determinism_and_no_sync():
    """10 poses at 96 x 96: device mse = host mse (relative 1e-9) per frame; the raw result blocks are bit-identical between 4 frames in
    flight and 1, and between two runs; SSIM equals the restatement on the host path's own rgb_map; and no evaluate() call of the device
    path synchronises (torch.cuda.set_sync_debug_mode('error') around each of them — see the last lines for what is done where the
    runtime does not honour the mode)."""
    from invr import driver
    net = _net(dict(table_log2=12, N_samples=64))
    seq = _sequence(10, 96)
    host = driver.run_evaluate(net, seq, device='cuda:0', in_flight=4, keep_maps=True)
    from invr.config import Node
    from invr.evaluator import Evaluator

    class NoSync(Evaluator):                       # every evaluate() of the device path under the synchronisation detector
        def evaluate(self, output, batch, epoch=-1):
            torch.cuda.set_sync_debug_mode('error')
            try:
                return super().evaluate(output, batch, epoch)
            finally:
                torch.cuda.set_sync_debug_mode('default')
    runs = []
    for K in (4, 1, 4):
        ev = NoSync(cfg=Node(test_full=True, fast_eval=True, dry_run=False, eval_part='', result_dir='unused'))
        out = driver.run_evaluate(net, seq, device='cuda:0', in_flight=K, metrics='device', evaluator=ev)
        out['blocks'] = ev.last_blocks.clone()
        assert out['blocks'].shape == (10, 64)
        runs.append(out)
    for f in range(10):
        assert rel(runs[0]['mse'][f], host['mse'][f]) <= 1e-9, f
        b = seq[f]
        H, W = int(b['H'].item()), int(b['W'].item())
        ref = R.frame_metrics(host['rgb_map'][f].numpy(), b['rgb'][0].numpy(), b['mask_at_box'][0].numpy(), H, W)
        assert abs(runs[0]['ssim'][f] - ref['ssim']) <= 1e-9, f
    for other in runs[1:]:
        assert torch.equal(runs[0]['blocks'], other['blocks'])                   # SSE, sum S, ... as bit patterns
        assert other['mse'] == runs[0]['mse'] and other['ssim'] == runs[0]['ssim']
    # does this runtime honour the mode at all?  A deliberate .item() on a device scalar must raise under 'error'.
    honoured = False
    torch.cuda.set_sync_debug_mode('error')
    try:
        torch.ones(1, device='cuda:0').sum().item()
    except RuntimeError:
        honoured = True
    finally:
        torch.cuda.set_sync_debug_mode('default')
    print('torch.cuda.set_sync_debug_mode honoured on this runtime:', honoured)
    assert honoured, 'set_sync_debug_mode is not honoured here: the no-synchronisation property was not checked'
