"""A training set that keeps a sequence on the device and forms every iteration's batch there: the patch branch of the reference's
dataset (lib/datasets/h36m/tpose_dataset.py:421-441, taken by every INB yaml: use_lpips, patch_size 64, sample_focus switched by the
training stages) without its per-iteration image I/O, NumPy ray pass, collation and host-to-device copy of the whole dict.

  add_frame   uploads a frame once: its pixels, its mask and its scene tensors (A, big_A, pbw, ...), and precomputes on the host what the
              window draw needs (the crop rectangles of crop_image_msk, row prefix counts of the mask's `== 1` pixels).
  draw        pure host code: crop_image_msk + random_crop_image (lib/utils/if_nerf/if_nerf_data_utils.py:611-686) with the reference's
              own random draws in its own order -> the window and its float32 intrinsic matrix.
  train_batch draw + ONE kernel launch (invr_patch_batch, include/invr_batch.h): the window's rays, the ones inside the body's box
              compacted in pixel order, the pixels and the mask gathered for them.  The batch references the resident scene tensors.
  batches     the same, `prefetch` batches ahead on a stream the set owns; yielding waits on that batch's event only.
  test_batch  the full-frame eval batch (rays.rays_within_bounds).

Not built (the reference's other sampling branches): the plain sample_ray_h36m branch (:228-310: cv2.fillPoly bound masks and a
resampling loop whose draws depend on device results), sample_using_mse, train_with_coord, prune_using_hull; image I/O and
undistortion (the host hands in frames as the reference holds them at tpose_dataset.py:351); a Dataset wrapper for the reference's
DataLoader."""
import contextlib
import ctypes as C
from collections import deque

import numpy as np
import torch

from . import _abi
from . import config as _config
from .config import PART_NAMES

MAX_SIDE = 256          # include/invr_batch.h INVR_PATCH_MAX_SIDE


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

    def add_frame(self, img, msk, K, R, T, scene, sem_masks=None, latent_index=None, frame_index=None, cam_ind=0):
        """img (H,W,3) float32 and msk (H,W) uint8 as the reference holds them at tpose_dataset.py:351 (undistorted, resized, mask_bkgd
        applied; mask values 0 / 1 / 100); K (3,3), R (3,3), T (3,1) the float64 camera (K scaled by cfg.ratio, T in metres); sem_masks
        (5,H,W) in PART_NAMES order; scene: the frame's un-batched item tensors (A, big_A, pbw, pbounds, wbounds, R, Th, ppts, part_pts,
        part_pbw, lengths2, bounds, ...), `wbounds` among them.  -> the frame's index."""
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

    def _finish(self, pending):
        """Join one pending batch (a host wait on ITS event only) and collate it: the first `count` rows of the compact tensors."""
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

    def train_batch(self, index, rng=None):
        """One training batch of frame `index`: the reference item's keys, collated (leading batch dimension of 1)."""
        return self._finish(self._submit(index, rng, self._slot()))

    def batches(self, order, rng=None, prefetch=2):
        """Generator over the batches of the frames in `order`, `prefetch` of them launched ahead on the set's own stream.  Yielding
        waits on the batch's own event on the host and makes the caller's current stream wait on it; the caller's stream is never
        synchronised.  The draws happen in `order`: the sequence of batches does not depend on `prefetch`.  A yielded batch's tensors
        are its own: it stays valid for as long as the caller holds it."""
        prefetch = max(0, int(prefetch))
        slots = deque(self._slot() for _ in range(prefetch + 1))
        queue = deque()
        for index in order:
            queue.append(self._submit(index, rng, slots.popleft()))
            if len(queue) > prefetch:
                pending = queue.popleft()
                batch = self._finish(pending)
                slots.append(pending[3])
                yield batch
        while queue:
            yield self._finish(queue.popleft())

    def batch_fn(self, order, rng=None, prefetch=2):
        """-> batch_fn(epoch, index) for driver.train(wrapper, optimizer, batch_fn, ...): the next batch of `order` per call."""
        it = self.batches(order, rng, prefetch)
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
