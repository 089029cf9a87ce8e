"""`Evaluator` with the surface of the reference's lib/evaluators/if_nerf.py, computing its per-frame image metrics (mse, psnr,
SSIM) on the device in float64 (invr.metrics over csrc/k_metrics.hip) without a host round trip per frame.

evaluate() enqueues two launches on the current stream and leaves the frame's 64-byte result block in a device-side ring; the values
are read back ONCE, in summarize() (or results() / collect()), where psnr is formed with the reference's own NumPy expression and the
reference's per-frame rules are applied:
  cfg.test_full True  (:80-127)  mse over the whole H x W frame, SSIM over the whole frame
  cfg.test_full False (:133-144) frames whose ground truth sums to 0 are skipped; mse over the rays inside the box; SSIM over the
                                 mask's bounding rectangle (:68-72) — a rectangle with a side below 7 pixels raises ValueError, as
                                 scikit-image does
  cfg.dry_run                    nothing is accumulated, summarize() returns None (:109-110, :150-151)
  cfg.fast_eval                  no images are written.  With fast_eval off the frame's two PNGs (names of :58-65) are written from the
                                 uint8 device image — a device-to-host copy per frame, the one place a frame waits for the device.  (The
                                 reference's test_full False branch writes them whatever fast_eval says; here fast_eval decides in both.)
  cfg.eval_part                  not built: raises at construction
LPIPS (:118-122, lp.LPIPS(net='vgg') on the two whole frames, cfg.test_full only) runs on the device too (invr.lpips_eval over
csrc/k_lpips.hip: a VGG16 forward of exact-fp32 matrix products, the distance in float64, bit-reproducible, no host round trip): its
device scalar joins the frame's pending results and is read back with them.  No weights ship here; at the first test_full frame they
are resolved from, in this order,
  1. Evaluator's lpips= argument: an invr.lpips_eval.LpipsVgg, or a module that is recognisably lpips.LPIPS(net='vgg')
  2. cfg.lpips_vgg16_weights + cfg.lpips_lin_weights: a torchvision VGG16 state dict and the lpips package's vgg.pth
  3. `import lpips` in the host process
A recognised module takes the device path unless cfg.eval_fused_lpips is False (then its own torch call runs, as does any module that
is not recognised).  The device path copies a module's weights and leaves the module alone; the torch call moves it to the frames'
device, puts it in eval mode and switches its gradients off, a module handed in as lpips= included.  The flag has no effect on an
LpipsVgg or on the two files: they have no torch call.  An argument or files that cannot be used raise.  With nothing available the list stays empty, the printed
summary omits it and a warning is issued once — no value is ever made up.
"""
import os
import sys
import warnings

import numpy as np
import torch

from . import metrics as M

RING_CHUNK = 256          # frames per block of the device-side result ring


def _cfg_get(cfg, key, default):
    if hasattr(cfg, 'get'):
        v = cfg.get(key, default)
    else:
        v = getattr(cfg, key, default)
    return default if v is None else v


def default_cfg():
    """The host application's parsed config (lib.config.cfg) when this process runs inside the reference, else invr.config.cfg."""
    host = sys.modules.get('lib.config')
    if host is not None and hasattr(host, 'cfg'):
        return host.cfg
    from . import config
    return config.cfg


_WRITER = False


def image_writer():
    """'cv2' / 'PIL' / None: what can write a PNG in this process"""
    global _WRITER
    if _WRITER is False:
        _WRITER = None
        for name in ('cv2', 'PIL.Image'):
            try:
                __import__(name)
                _WRITER = name.split('.')[0]
                break
            except ImportError:
                pass
    return _WRITER


def write_png(path, bgr_u8):
    """(H,W,3) uint8 in B,G,R order -> PNG, as cv2.imwrite stores it"""
    w = image_writer()
    if w == 'cv2':
        import cv2
        cv2.imwrite(path, bgr_u8)
    elif w == 'PIL':
        from PIL import Image
        Image.fromarray(np.ascontiguousarray(bgr_u8[..., ::-1])).save(path)
    else:
        raise RuntimeError('Evaluator: cfg.fast_eval is off but neither cv2 nor PIL can be imported to write %s' % path)


def fill_image(img, batch):
    """if_nerf.py:183-191 on the uint8 image: paste the cropped render into the original-size frame"""
    orig_H, orig_W = int(batch['orig_H'].item()), int(batch['orig_W'].item())
    full = np.zeros((orig_H, orig_W, 3), dtype=img.dtype)
    bbox = batch['crop_bbox'][0].detach().cpu().numpy()
    height, width = bbox[1, 1] - bbox[0, 1], bbox[1, 0] - bbox[0, 0]
    full[bbox[0, 1]:bbox[1, 1], bbox[0, 0]:bbox[1, 0]] = img[:height, :width]
    return full


class Evaluator:
    def __init__(self, cfg=None, lpips=None):
        self.cfg = default_cfg() if cfg is None else cfg
        self._lpips_arg = lpips          # an LpipsVgg, a torch module, or None
        if _cfg_get(self.cfg, 'eval_part', '') != '':
            raise ValueError('invr: unsupported configuration eval_part = %r — the per-part evaluation mask (if_nerf.py:91-94) is not built'
                             % (_cfg_get(self.cfg, 'eval_part', ''),))
        self.mse, self.psnr, self.ssim, self.lpips = [], [], [], []
        self.last_blocks = None          # host copy of the result blocks of the last read-back, (frames, 64) uint8
        self._ring = []                  # device tensors (RING_CHUNK, 64) uint8
        self._frames = []                # (H, W, test_full) per pending frame, in ring order
        self._lpips_dev = []             # device scalars of the pending test_full frames: float64 of the device path, float32 of the torch call
        self._read = None                # decoded blocks of the pending frames once read back
        self._ws = {}                    # (device, stream) -> (H, W, workspace)
        self._loss_fn = None             # the torch module of the torch path
        self._lpips_fused = None         # the LpipsVgg of the device path
        self._lpips_state = None         # None = not tried, True / False

    # ---- switches (read at every call: the reference reads the global cfg) ----
    test_full = property(lambda s: bool(_cfg_get(s.cfg, 'test_full', True)))
    fast_eval = property(lambda s: bool(_cfg_get(s.cfg, 'fast_eval', False)))
    dry_run = property(lambda s: bool(_cfg_get(s.cfg, 'dry_run', False)))
    result_dir = property(lambda s: str(_cfg_get(s.cfg, 'result_dir', 'exps')))

    def psnr_metric(self, img_pred, img_gt):
        mse = np.mean((img_pred - img_gt) ** 2)
        return M.psnr_of(mse)

    def _workspace(self, H, W, device):
        key = (str(device), M._abi.stream_ptr().value)
        have = self._ws.get(key)
        if have is None or have[0] < H or have[1] < W:          # grow-only: a workspace for (h, w) serves every frame up to h x w
            h, w = max(H, have[0] if have else 0), max(W, have[1] if have else 0)
            have = self._ws[key] = (h, w, M.new_workspace(h, w, device))
        return have[2]

    def _slot(self, device):
        k = len(self._frames)
        if k // RING_CHUNK >= len(self._ring):
            self._ring.append(M.new_results(RING_CHUNK, device))
        return self._ring[k // RING_CHUNK][k % RING_CHUNK]

    def _lpips_resolve(self, device):
        """-> (LpipsVgg or None, torch module or None) by the order of the module docstring; (None, None) after the one warning when
        nothing is available.  What the caller NAMED — the argument, the two files — raises if it cannot be used."""
        from . import lpips_eval
        fused = bool(_cfg_get(self.cfg, 'eval_fused_lpips', True))
        arg = self._lpips_arg
        if isinstance(arg, lpips_eval.LpipsVgg):
            return arg, None
        module = arg
        if module is None:
            vgg, lin = _cfg_get(self.cfg, 'lpips_vgg16_weights', None), _cfg_get(self.cfg, 'lpips_lin_weights', None)
            if vgg and lin:
                return lpips_eval.LpipsVgg.from_files(vgg, lin, device=device), None
            try:
                import lpips as lp
                module = lp.LPIPS(net='vgg', verbose=False)
            except Exception as e:          # the package, or its weights, are not there
                warnings.warn('invr Evaluator: LPIPS is not computed (%s: %s); the lpips list stays empty' % (type(e).__name__, e))
                return None, None
        net = lpips_eval.LpipsVgg.from_module(module, device=device) if fused else None      # (copies the weights: the module stays as it is)
        if net is not None:
            return net, None
        module = module.to(device).eval()          # the torch path calls the module itself: moved, eval mode, no gradients — the caller's too
        for p in module.parameters():
            p.requires_grad_(False)
        return None, module

    def _lpips(self, img_pred, img_gt):
        if self._lpips_state is None:
            self._lpips_fused, self._loss_fn = self._lpips_resolve(img_pred.device)
            self._lpips_state = self._lpips_fused is not None or self._loss_fn is not None
        if self._lpips_state:
            if self._lpips_fused is not None:
                self._lpips_dev.append(self._lpips_fused(img_pred, img_gt))
            else:
                with torch.no_grad():
                    self._lpips_dev.append(self._loss_fn(img_pred.permute(2, 0, 1)[None], img_gt.permute(2, 0, 1)[None])[0].detach())

    def _write_images(self, u8_pred, u8_gt, batch, epoch):
        result_dir = os.path.join(self.result_dir, 'comparison_epoch%d' % epoch if epoch != -1 else 'comparison')
        os.makedirs(result_dir, exist_ok=True)
        frame_index, view_index = int(batch['frame_index'].item()), int(batch['cam_ind'].item())
        for u8, tail in ((u8_pred, ''), (u8_gt, '_gt')):
            img = u8.cpu().numpy()
            if 'crop_bbox' in batch:
                img = fill_image(img, batch)
            write_png('{}/frame{:04d}_view{:04d}{}.png'.format(result_dir, frame_index, view_index, tail), img)

    def evaluate(self, output, batch, epoch=-1):
        """output['rgb_map'] (1,n,3): a device tensor (used in place) or a host tensor (uploaded, non-blocking); batch: 'rgb' (1,n,3),
        'mask_at_box' (1,H*W), 'H', 'W' (+ 'frame_index', 'cam_ind' when images are written).  H and W are read with .item(): keep
        them on the host (driver.run_evaluate does) or that read is a synchronisation."""
        test_full, fast_eval, dry_run = self.test_full, self.fast_eval, self.dry_run
        if dry_run and fast_eval:
            return
        rgb_pred = output['rgb_map'][0].detach()
        rgb_gt = batch['rgb'][0].detach()
        mask = batch['mask_at_box'][0].detach()
        device = rgb_pred.device
        for t in (rgb_gt, mask):                       # an uploaded render is evaluated where the batch lives
            if device.type == 'cpu' and t.device.type != 'cpu':
                device = t.device
        H, W = int(batch['H'].item()), int(batch['W'].item())
        self._read = None
        slot = self._slot(device) if not dry_run else M.new_results(1, device)[0]
        ws = self._workspace(H, W, device)
        img_pred, img_gt, u8_pred, u8_gt = M.image_assemble(rgb_pred, rgb_gt, mask, H, W, slot, ws, want_u8=not fast_eval)
        if not fast_eval:
            self._write_images(u8_pred, u8_gt, batch, epoch)
        if dry_run:
            return
        M.image_metrics(img_pred, img_gt, slot, ws, crop=not test_full)
        self._frames.append((H, W, test_full))
        if test_full:                                  # (:118-122: the reference computes LPIPS in this branch only)
            self._lpips(img_pred, img_gt)

    def results(self):
        """The pending frames' result blocks, decoded (invr.metrics.decode) — the one read-back; repeated calls reuse it."""
        if self._read is None:
            n = len(self._frames)
            if n == 0:
                self.last_blocks = torch.zeros((0, M.RESULT_BYTES), dtype=torch.uint8)
                self._read = []
            else:
                chunks = [r.cpu() for r in self._ring[:(n + RING_CHUNK - 1) // RING_CHUNK]]
                self.last_blocks = torch.cat(chunks)[:n].contiguous()
                self._read = [M.decode(self.last_blocks[k]) for k in range(n)]
        return list(self._read)

    def collect(self):
        """Read the pending frames back, apply the reference's per-frame rules and append to the mse / psnr / ssim / lpips lists."""
        res = self.results()
        lp = [float(v) for v in torch.stack(self._lpips_dev).reshape(-1).cpu()] if self._lpips_dev else []
        frames, self._frames, self._lpips_dev, self._read = self._frames, [], [], None
        lp_at = 0
        for k, (r, (H, W, test_full)) in enumerate(zip(res, frames)):
            if r['status'] != 0:
                raise RuntimeError('invr Evaluator: frame %d: mask_at_box has %d set entries, rgb_map has another number of rows' % (k, r['n_set']))
            if test_full:
                lpips_k = lp[lp_at] if lp_at < len(lp) else None
                lp_at += 1
            elif r['sum_gt'] == 0:                     # (:134-135)
                continue
            mse = M.mse_of(r, H, W, test_full)
            ssim = M.ssim_of(r)                        # ValueError when the image / rectangle has no window
            self.mse.append(mse)
            with np.errstate(divide='ignore'):
                self.psnr.append(M.psnr_of(mse))
            self.ssim.append(ssim)
            if test_full and lpips_k is not None:
                self.lpips.append(lpips_k)

    def summarize(self, epoch=-1):
        if self.fast_eval:
            print('WARNING: only saving evaluation metrics, no images will be saved!')
        if self.dry_run:
            self._frames, self._lpips_dev, self._read = [], [], None
            return None
        self.collect()
        result_dir = self.result_dir
        print('the results are saved at {}'.format(result_dir))
        result_path = os.path.join(result_dir, 'metrics.npy' if epoch == -1 else 'metrics_epoch{}.npy'.format(epoch))
        os.makedirs(os.path.dirname(result_path) or '.', exist_ok=True)
        np.save(result_path, {'mse': self.mse, 'psnr': self.psnr, 'ssim': self.ssim, 'lpips': self.lpips})
        ret = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)          # (np.mean of an empty list, as in the reference)
            print('mse: {}'.format(np.mean(self.mse)))
            print('psnr: {}'.format(np.mean(self.psnr)))
            print('ssim: {}'.format(np.mean(self.ssim)))
            ret.update({'psnr': np.mean(self.psnr), 'ssim': np.mean(self.ssim)})
            if self.lpips:
                print('lpips: {}'.format(np.mean(self.lpips)))
                ret['lpips'] = np.mean(self.lpips)
        self.mse, self.psnr, self.ssim, self.lpips = [], [], [], []
        return ret
