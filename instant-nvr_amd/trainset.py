"""A training set that keeps a sequence on the device and forms every iteration's batch there, without the reference's per-iteration
image I/O, NumPy ray pass, collation and host-to-device copy of the whole dict.  Two branches of its Dataset.__getitem__:
the patch branch (lib/datasets/h36m/tpose_dataset.py:421-441, taken by every INB yaml: use_lpips, patch_size 64, sample_focus switched
by the training stages) and the plain branch (:442-450, taken when none of use_lpips / patch_sampling / use_ssim / use_fourier /
use_tv_image is set: cfg.N_rand rays drawn from the body mask, the face mask and the projected box by sample_ray_h36m).

  add_frame   uploads a frame once: its pixels, its mask and its scene tensors (A, big_A, pbw, ...), and precomputes on the host what the
              window draw needs (the crop rectangles of crop_image_msk, row prefix counts of the mask's `== 1` pixels).  With `orig_msk`
              it also prepares plain sampling (invr.raysample): the bound mask, the three pixel classes as bit planes + row prefix
              counts on the device, and per class member the reference's own mask_at_box decision on the host.
  draw        pure host code: crop_image_msk + random_crop_image (lib/utils/if_nerf/if_nerf_data_utils.py:611-686) with the reference's
              own random draws in its own order -> the window and its float32 intrinsic matrix.
  draw_rays   pure host code: the sampling loop of sample_ray_h36m (:253-289) with its randint calls in its order -> (class, rank) rows.
  train_batch patch: draw + ONE kernel launch (invr_patch_batch, include/invr_batch.h): the window's rays, the ones inside the body's
              box compacted in pixel order, the pixels and the mask gathered for them.  plain: draw_rays + ONE kernel launch
              (invr_ray_batch, include/invr_sample.h).  The batch references the resident scene tensors.
  batches     the same, `prefetch` batches ahead on a stream the set owns; yielding waits on that batch's event only.
  test_batch  the full-frame eval batch (rays.rays_within_bounds).

`mode` of the batch calls: 'patch', 'plain', or None = the reference's rule at :421 read from cfg per batch (a frame that was added
without `orig_msk` can only give patches and does so under None, as before plain sampling existed; mode='plain' raises for it).

The two branches collate differently, as the reference does: a plain batch has coord (1,n,2) int64 (row, col) where a patch has uint8
(x, y) of the window, occupancy (1,n) uint8 = orig_msk at the pixel where a patch has bool, mask_at_box all True of n entries, and H, W
of the frame.

Not built (the reference's other sampling branches): sample_using_mse, train_with_coord, prune_using_hull / prune_using_geo (plain
sampling raises when cfg sets one); image I/O, undistortion and crop_mask_edge (the host hands in frames as the reference holds them at
tpose_dataset.py:351, and orig_msk as it reads it at :450); a Dataset wrapper for the reference's DataLoader."""
import contextlib
import ctypes as C
from collections import deque

import numpy as np
import torch

from . import _abi
from . import config as _config
from . import raysample
from .config import PART_NAMES

MAX_SIDE = 256          # include/invr_batch.h INVR_PATCH_MAX_SIDE
MAX_RAYS = 1 << 20      # include/invr_sample.h INVR_RAY_BATCH_MAX
STAGING = 4             # page-locked buffers the (class, rank) rows of plain batches travel through


def bounding_rect(mask):
    """cv2.boundingRect of a single-channel mask restated: (x, y, w, h) of its non-zero pixels, zeros when there are none."""
    rows, cols = np.flatnonzero(mask.any(1)), np.flatnonzero(mask.any(0))
    if len(rows) == 0:
        return 0, 0, 0, 0
    return int(cols[0]), int(rows[0]), int(cols[-1] - cols[0] + 1), int(rows[-1] - rows[0] + 1)


def padding_bbox(x, y, w, h, H, W):
    """padding_bbox (:580-608) of [[x, y], [x + w, y + h]] in an H x W image -> (x_lo, y_lo, x_hi, y_hi), hi exclusive."""
    x_lo, y_lo, x_hi, y_hi = x - 10, y - 10, x + w + 10, y + h + 10
    height, width = y_hi - y_lo, x_hi - x_lo
    if height / width > 1.5 and width < int(height / 1.5):
        pad = (int(height / 1.5) - width) // 2
        x_lo, x_hi = x_lo - pad, x_hi + pad
    if width / height > 1.5 and height < int(width / 1.5):
        pad = (int(width / 1.5) - height) // 2
        y_lo, y_hi = y_lo - pad, y_hi + pad
    clip = lambda v, hi: min(max(v, 0), hi)
    return clip(x_lo, W - 1), clip(y_lo, H - 1), clip(x_hi, W - 1), clip(y_hi, H - 1)


class _Crop:
    """One candidate crop of a frame: the reference mask's bounding rectangle (for the `None` rule of crop_image_msk :613-614), the
    padded rectangle, and per row of it the number of `msk == 1` pixels before that row (what finds the k-th one in row-major order)."""

    def __init__(self, msk, ref):
        H, W = msk.shape
        x, y, self.w, self.h = bounding_rect(ref)
        self.rect = padding_bbox(x, y, self.w, self.h, H, W) if self.w and self.h else (0, 0, 0, 0)
        self.rows = self.prefix(msk, self.rect)

    @staticmethod
    def prefix(msk, rect):
        x_lo, y_lo, x_hi, y_hi = rect
        return np.concatenate([[0], np.cumsum((msk[y_lo:y_hi, x_lo:x_hi] == 1).sum(1, dtype=np.int64))])


class _Frame:
    pass


class TrainSet:
    def __init__(self, cfg=None, device='cuda', shared=None):
        self.cfg = _config.cfg if cfg is None else cfg
        self.device = torch.device(device)
        self.frames = []
        self.shared = {}
        self._stream = None                 # the side stream the batches are formed on (created with the first batch)
        self._uploaded = None               # event behind the last upload: the side stream waits on it
        self._staging, self._staged = [], 0   # the ring of [pinned (cap,2) int32 buffer, event behind its last copy]
        self._true_rows = None              # mask_at_box of plain batches: constant rows every such batch views
        if shared:
            self.set_shared(shared)

    def __len__(self):
        return len(self.frames)

    # ---- filling ------------------------------------------------------------------------------------------------------------------
    def _upload(self, v):
        """One item of the reference's dataset -> the collated tensor (leading batch dimension of 1) on the device."""
        if not torch.is_tensor(v):
            v = np.asarray(v)
            v = torch.from_numpy(v if v.flags.c_contiguous else np.ascontiguousarray(v))
        return v.to(self.device)[None].contiguous()

    def _mark_uploaded(self):
        if self.device.type == 'cuda':
            self._uploaded = torch.cuda.Event()
            self._uploaded.record(torch.cuda.current_stream(self.device))

    def set_shared(self, shared):
        """What every frame shares (tbw, tuv, tbounds, ...): un-batched arrays, uploaded once."""
        self.shared = {k: self._upload(v) for k, v in shared.items()}
        self._mark_uploaded()

    def add_frame(self, img, msk, K, R, T, scene, sem_masks=None, latent_index=None, frame_index=None, cam_ind=0, orig_msk=None,
                  bound_mask=None, face_value=13):
        """img (H,W,3) float32 and msk (H,W) uint8 as the reference holds them at tpose_dataset.py:351 (undistorted, resized, mask_bkgd
        applied; mask values 0 / 1 / 100); K (3,3), R (3,3), T (3,1) the float64 camera (K scaled by cfg.ratio, T in metres); sem_masks
        (5,H,W) in PART_NAMES order; scene: the frame's un-batched item tensors (A, big_A, pbw, pbounds, wbounds, R, Th, ppts, part_pts,
        part_pbw, lengths2, bounds, ...), `wbounds` among them.  -> the frame's index.
        Plain sampling needs orig_msk (H,W) uint8: the mask the reference reads `occupancy` from (tpose_dataset.py:450, crop_mask_edge
        already applied when cfg.erode_edge).  bound_mask (H,W) of 0 / 1 is the host's get_bound_2d_mask for pixel parity with cv2; by
        default the set fills the hull of the projected box itself (raysample.bound_mask: may differ from cv2 on the hull's outline).
        face_value is the mask value of the face class (`msk == 13`)."""
        img, msk = np.array(img, np.float32, order='C'), np.array(msk, np.uint8, order='C')          # copies: the caller may reuse its buffers
        if img.ndim != 3 or img.shape[2] != 3 or msk.shape != img.shape[:2]:
            raise ValueError('add_frame: img must be (H, W, 3) and msk (H, W) (got %s and %s)' % (img.shape, msk.shape))
        if 'wbounds' not in scene:
            raise ValueError("add_frame: scene['wbounds'], the world box of the frame's body, is missing")
        f = _Frame()
        f.index = len(self.frames)
        f.H, f.W = msk.shape
        f.msk_host = msk
        f.K, f.R, f.T = np.array(K, np.float64).reshape(3, 3), np.array(R, np.float64).reshape(3, 3), np.array(T, np.float64).reshape(3, 1)
        f.cam_o = -np.dot(f.R.T, f.T).ravel()                              # get_rays_coord :43
        f.Tr = np.ascontiguousarray(f.T.ravel())
        wb = scene['wbounds']
        f.wbounds = np.ascontiguousarray(wb.detach().cpu().numpy() if torch.is_tensor(wb) else wb, np.float32).reshape(6)
        f.full = (0, 0, f.W, f.H)
        f.full_rows = _Crop.prefix(msk, f.full)
        f.crops = {'': _Crop(msk, msk)}
        if sem_masks is not None:
            sem_masks = np.asarray(sem_masks)
            if sem_masks.shape != (len(PART_NAMES),) + msk.shape:
                raise ValueError('add_frame: sem_masks must be (%d, H, W) in PART_NAMES order (got %s)' % (len(PART_NAMES), sem_masks.shape))
            for name, sm in zip(PART_NAMES, sem_masks):
                if sm.sum() != 0:                                              # an empty semantic mask falls back to msk (:424)
                    f.crops[name] = _Crop(msk, sm)
        f.has_sem = sem_masks is not None
        f.classes = None
        if orig_msk is not None:
            orig_msk = np.array(orig_msk, np.uint8, order='C')
            if orig_msk.shape != msk.shape:
                raise ValueError('add_frame: orig_msk must be (H, W) like msk (got %s)' % (orig_msk.shape,))
            if bound_mask is None:
                bound_mask = raysample.bound_mask(f.wbounds, f.K, f.R, f.T, f.H, f.W)
            else:
                bound_mask = np.asarray(bound_mask)
                if bound_mask.shape != msk.shape or not np.isin(bound_mask, (0, 1)).all():
                    raise ValueError('add_frame: bound_mask must be (H, W) of 0 / 1 as get_bound_2d_mask returns it')
            f.classes = raysample.FrameClasses(msk, bound_mask, raysample.inside_box(f.H, f.W, f.K, f.R, f.T, f.wbounds), face_value)
            f.k_inv = np.ascontiguousarray(np.linalg.inv(f.K))                  # get_rays :32, float64
            f.orig_msk = torch.from_numpy(orig_msk).to(self.device)
            f.planes = torch.from_numpy(f.classes.planes.view(np.int64)).to(self.device)
            f.row_prefix = torch.from_numpy(f.classes.row_prefix).to(self.device)
        elif bound_mask is not None:
            raise ValueError('add_frame: bound_mask is given without orig_msk: it serves plain sampling only')
        latent_index = f.index if latent_index is None else int(latent_index)
        frame_index = latent_index if frame_index is None else int(frame_index)
        f.img = torch.from_numpy(img).to(self.device)
        f.msk = torch.from_numpy(msk).to(self.device)
        f.ray_o = torch.from_numpy(f.cam_o.astype(np.float32)).to(self.device)
        f.ray_o_rows = f.ray_o[None].expand(MAX_SIDE * MAX_SIDE, 3).contiguous()         # constant rows every batch of the frame views
        f.scene = {k: self._upload(v) for k, v in scene.items()}
        ntf = float(self.cfg.get('num_train_frame', 100))
        f.meta = {'frame_dim': self._upload(np.array(latent_index / ntf).astype(np.float32)),           # :497
                  'latent_index': self._upload(np.int64(latent_index)), 'bw_latent_index': self._upload(np.int64(latent_index)),
                  'frame_index': torch.tensor([frame_index], dtype=torch.int64), 'cam_ind': torch.tensor([int(cam_ind)], dtype=torch.int64)}
        self.frames.append(f)
        self._mark_uploaded()
        return f.index

    # ---- the window draw (host) ---------------------------------------------------------------------------------------------------
    def draw(self, index, rng=None):
        """-> (x0, y0, w, h, K32): crop_image_msk + random_crop_image on frame `index` with the reference's draws in its order (the side,
        then the centre pixel) from rng (np.random.RandomState; None = the global np.random, as the reference).  The window is in
        frame coordinates; K32 is its float32 intrinsic matrix.  cfg.patch_size and cfg.sample_focus are read now."""
        rng = np.random if rng is None else rng
        f = self.frames[index]
        patch, focus = int(self.cfg.patch_size), self.cfg.get('sample_focus', '') or ''
        if focus != '' and not f.has_sem:
            raise ValueError('TrainSet.draw: cfg.sample_focus = %r but frame %d was added without sem_masks' % (focus, index))
        if focus != '' and focus not in PART_NAMES:
            raise ValueError('TrainSet.draw: cfg.sample_focus = %r is none of %s' % (focus, PART_NAMES))
        crop = f.crops.get(focus, f.crops[''])
        K = f.K.copy()
        if crop.w < patch or crop.h < patch:                                   # crop_image_msk returned None: the whole frame, K stays float64
            rect, rows = f.full, f.full_rows
        else:
            rect, rows = crop.rect, crop.rows
            K[0, 2] -= rect[0]
            K[1, 2] -= rect[1]
            K = K.astype(np.float32)
        x_lo, y_lo, x_hi, y_hi = rect
        H, W = y_hi - y_lo, x_hi - x_lo
        m = min(H, W, patch)
        size = (int(rng.randint(int(min(patch, 0.8 * m)), m)) | 7) + 1
        if size > H or size > W:
            raise ValueError('TrainSet.draw: frame %d: a %d x %d window does not fit its %d x %d crop (cfg.patch_size = %d)'
                             % (index, size, size, W, H, patch))
        k = int(rng.randint(0, int(rows[-1])))                                 # the k-th `msk == 1` pixel of the crop, row-major
        r = int(np.searchsorted(rows, k, side='right')) - 1
        cy, cx = r, int(np.flatnonzero(f.msk_host[y_lo + r, x_lo:x_hi] == 1)[k - int(rows[r])])
        x, y = cx - size // 2, cy - size // 2
        x = 0 if x < 0 else x
        x = W - size if x + size > W else x
        y = 0 if y < 0 else y
        y = H - size if y + size > H else y
        K[0, 2] = K[0, 2] - x
        K[1, 2] = K[1, 2] - y
        return x_lo + x, y_lo + y, size, size, K.astype(np.float32)

    # ---- the ray draw of the plain branch (host) ----------------------------------------------------------------------------------
    def draw_rays(self, index, rng=None):
        """-> sel (n,2) int32 (class, rank): the sampling loop of sample_ray_h36m on frame `index` with the reference's randint calls in
        its order from rng (None = the global np.random).  n >= cfg.N_rand and rows repeat, as in the reference.  cfg.N_rand,
        cfg.body_sample_ratio and cfg.face_sample_ratio are read now."""
        f = self.frames[index]
        if f.classes is None:
            raise ValueError('TrainSet: plain sampling on frame %d, which was added without orig_msk' % index)
        _config.check_plain_sampling(self.cfg)
        sel = raysample.draw_rays(f.classes, self.cfg.get('N_rand', 1024), self.cfg.get('body_sample_ratio', 0.5),
                                  self.cfg.get('face_sample_ratio', 0.0), rng, frame=index)
        if len(sel) > MAX_RAYS:
            raise ValueError('TrainSet.draw_rays: %d rays are beyond the %d of one invr_ray_batch call' % (len(sel), MAX_RAYS))
        return sel

    def _mode(self, mode, index):
        """'patch' or 'plain' for a batch of frame `index`; None = tpose_dataset.py:421 on cfg as it stands now."""
        if mode is None:
            patch = any(bool(self.cfg.get(k, False)) for k in _config.PATCH_FLAGS) or self.frames[index].classes is None
            return 'patch' if patch else 'plain'
        if mode not in ('patch', 'plain'):
            raise ValueError("TrainSet: mode must be 'patch', 'plain' or None (got %r)" % (mode,))
        return mode

    # ---- batches --------------------------------------------------------------------------------------------------------------------
    def _side(self):
        if self.device.type != 'cuda':
            return None
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
        return self._stream

    def _submit(self, index, rng, slot):
        """Draw and launch one batch on the side stream; its count goes to the pinned `slot` asynchronously.  -> the pending batch."""
        f = self.frames[index]
        x0, y0, w, h, K32 = self.draw(index, rng)
        k_inv = np.ascontiguousarray(np.linalg.inv(K32), np.float32)          # get_rays_coord :53, float32 by then
        n = w * h
        side = self._side()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if side is not None and self._uploaded is not None:
                side.wait_event(self._uploaded)
            dev = self.device
            o = {'ray_d': torch.empty(n, 3, device=dev), 'near': torch.empty(n, device=dev), 'far': torch.empty(n, device=dev),
                 'rgb': torch.empty(n, 3, device=dev), 'occupancy': torch.empty(n, dtype=torch.uint8, device=dev),
                 'coord': torch.empty(n, 2, dtype=torch.uint8, device=dev), 'mask_at_box': torch.empty(n, dtype=torch.uint8, device=dev)}
            count = torch.empty(1, dtype=torch.int32, device=dev)
            u8 = torch.uint8
            st = C.c_void_p(side.cuda_stream) if side is not None else _abi.stream_ptr()
            _abi.check(_abi.lib().invr_patch_batch(
                _abi.ptr(f.img), _abi.ptr(f.msk, u8), f.H, f.W, x0, y0, w, h, fp(k_inv), dp(np.ascontiguousarray(f.R)), dp(f.Tr), dp(f.cam_o),
                fp(f.wbounds), _abi.ptr(o['ray_d']), _abi.ptr(o['near']), _abi.ptr(o['far']), _abi.ptr(o['rgb']), _abi.ptr(o['occupancy'], u8),
                _abi.ptr(o['coord'], u8), _abi.ptr(o['mask_at_box'], u8), _abi.ptr(count, torch.int32), st))
            event = None
            if side is not None:
                slot.copy_(count, non_blocking=True)
                event = torch.cuda.Event()
                event.record(side)
            else:
                slot.copy_(count)
        return f, o, (w, h), slot, event

    def _stage(self, sel):
        """The (class, rank) rows on the device, through the next page-locked buffer of the ring (on the side stream).  A buffer is
        written again only after the copy that last read it has finished."""
        sel = torch.from_numpy(sel)
        if self.device.type != 'cuda':
            return sel, None
        if len(self._staging) < STAGING:
            self._staging.append([None, None])
        entry = self._staging[self._staged % len(self._staging)]
        self._staged += 1
        if entry[1] is not None:
            entry[1].synchronize()
        if entry[0] is None or entry[0].shape[0] < sel.shape[0]:
            entry[0] = torch.empty(max(sel.shape[0], 2048), 2, dtype=torch.int32, pin_memory=True)
        entry[0][:sel.shape[0]].copy_(sel)
        dev = torch.empty(sel.shape[0], 2, dtype=torch.int32, device=self.device)
        dev.copy_(entry[0][:sel.shape[0]], non_blocking=True)
        return dev, entry

    def _submit_plain(self, index, rng):
        """Draw and launch one plain batch on the side stream.  -> the pending batch; its size is known here."""
        f = self.frames[index]
        sel = self.draw_rays(index, rng)
        n = len(sel)
        side = self._side()
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            if side is not None and self._uploaded is not None:
                side.wait_event(self._uploaded)
            dev = self.device
            sel_d, entry = self._stage(sel)
            o = {'ray_d': torch.empty(n, 3, device=dev), 'near': torch.empty(n, device=dev), 'far': torch.empty(n, device=dev),
                 'rgb': torch.empty(n, 3, device=dev), 'occupancy': torch.empty(n, dtype=torch.uint8, device=dev),
                 'coord': torch.empty(n, 2, dtype=torch.int64, device=dev)}
            u8, i32, i64 = torch.uint8, torch.int32, torch.int64
            st = C.c_void_p(side.cuda_stream) if side is not None else _abi.stream_ptr()
            _abi.check(_abi.lib().invr_ray_batch(
                _abi.ptr(f.img), _abi.ptr(f.orig_msk, u8), _abi.ptr(f.planes, i64), _abi.ptr(f.row_prefix, i32), f.H, f.W, _abi.ptr(sel_d, i32), n,
                dp(f.k_inv), dp(np.ascontiguousarray(f.R)), dp(f.Tr), dp(f.cam_o), f.wbounds.ctypes.data_as(C.POINTER(C.c_float)),
                _abi.ptr(o['ray_d']), _abi.ptr(o['near']), _abi.ptr(o['far']), _abi.ptr(o['rgb']), _abi.ptr(o['occupancy'], u8),
                _abi.ptr(o['coord'], i64), st))
            event = None
            if side is not None:
                event = torch.cuda.Event()
                event.record(side)
                entry[1] = event
                sel_d.record_stream(side)
        return 'plain', f, o, n, event

    def _finish_plain(self, pending):
        """Collate one pending plain batch: the caller's stream waits on its event; the host does not (n is known)."""
        _, f, o, n, event = pending
        if event is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(event)
            for t in o.values():
                t.record_stream(cur)
        if f.ray_o_rows.shape[0] < n:                                              # constant rows: grown, never shrunk
            f.ray_o_rows = f.ray_o[None].expand(n, 3).contiguous()
        if self._true_rows is None or self._true_rows.shape[0] < n:
            self._true_rows = torch.ones(max(n, 4096), dtype=torch.bool, device=self.device)
        batch = {'rgb': o['rgb'][None], 'occupancy': o['occupancy'][None], 'coord': o['coord'][None], 'ray_o': f.ray_o_rows[None, :n],
                 'ray_d': o['ray_d'][None], 'near': o['near'][None], 'far': o['far'][None], 'mask_at_box': self._true_rows[None, :n],
                 'H': torch.tensor([f.H], dtype=torch.int64), 'W': torch.tensor([f.W], dtype=torch.int64)}
        batch.update(f.meta)
        batch.update(self.shared)
        batch.update(f.scene)
        return batch

    def _finish(self, pending):
        """Join one pending batch (a host wait on ITS event only) and collate it: the first `count` rows of the compact tensors."""
        if pending[0] == 'plain':
            return self._finish_plain(pending)
        f, o, (w, h), slot, event = pending
        if event is not None:
            event.synchronize()
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(event)
            for t in o.values():
                t.record_stream(cur)
        n = int(slot[0])
        batch = {'rgb': o['rgb'][None, :n], 'occupancy': o['occupancy'][None, :n].view(torch.bool), 'coord': o['coord'][None, :n],
                 'ray_o': f.ray_o_rows[None, :n], 'ray_d': o['ray_d'][None, :n], 'near': o['near'][None, :n], 'far': o['far'][None, :n],
                 'mask_at_box': o['mask_at_box'][None].view(torch.bool),
                 'H': torch.tensor([h], dtype=torch.int64), 'W': torch.tensor([w], dtype=torch.int64)}
        batch.update(f.meta)
        batch.update(self.shared)
        batch.update(f.scene)
        return batch

    def _slot(self):
        return torch.empty(1, dtype=torch.int32, pin_memory=self.device.type == 'cuda')

    def train_batch(self, index, rng=None, mode=None):
        """One training batch of frame `index`: the reference item's keys, collated (leading batch dimension of 1)."""
        if self._mode(mode, index) == 'plain':
            return self._finish(self._submit_plain(index, rng))
        return self._finish(self._submit(index, rng, self._slot()))

    def batches(self, order, rng=None, prefetch=2, mode=None):
        """Generator over the batches of the frames in `order`, `prefetch` of them launched ahead on the set's own stream.  Yielding
        waits on the batch's own event on the host and makes the caller's current stream wait on it; the caller's stream is never
        synchronised.  The draws happen in `order`: the sequence of batches does not depend on `prefetch`.  A yielded batch's tensors
        are its own: it stays valid for as long as the caller holds it.  `mode` is resolved per batch (None: from cfg as it stands then)."""
        prefetch = max(0, int(prefetch))
        slots = deque(self._slot() for _ in range(prefetch + 1))
        queue = deque()
        for index in order:
            if self._mode(mode, index) == 'plain':
                queue.append(self._submit_plain(index, rng))
            else:
                queue.append(self._submit(index, rng, slots.popleft() if slots else self._slot()))
            if len(queue) > prefetch:
                pending = queue.popleft()
                batch = self._finish(pending)
                if pending[0] != 'plain':
                    slots.append(pending[3])
                yield batch
        while queue:
            yield self._finish(queue.popleft())

    def batch_fn(self, order, rng=None, prefetch=2, mode=None):
        """-> batch_fn(epoch, index) for driver.train(wrapper, optimizer, batch_fn, ...): the next batch of `order` per call."""
        it = self.batches(order, rng, prefetch, mode)
        return lambda epoch, index: next(it)

    def test_batch(self, index):
        """The full-frame eval batch of frame `index` (rays.rays_within_bounds and the frame's pixels inside the box), for
        driver.run_evaluate(net, (ts.test_batch(i) for i in ...))."""
        from . import rays
        f = self.frames[index]
        ray_o, ray_d, near, far, mask = rays.rays_within_bounds(f.H, f.W, f.K, f.R, f.T, f.wbounds.reshape(2, 3), self.device)
        batch = {'rgb': f.img[mask][None], 'occupancy': (f.msk[mask] > 0)[None], 'ray_o': ray_o[None], 'ray_d': ray_d[None], 'near': near[None],
                 'far': far[None], 'mask_at_box': mask.reshape(1, -1),
                 'H': torch.tensor([f.H], dtype=torch.int64), 'W': torch.tensor([f.W], dtype=torch.int64)}
        batch.update(f.meta)
        batch.update(self.shared)
        batch.update(f.scene)
        return batch
