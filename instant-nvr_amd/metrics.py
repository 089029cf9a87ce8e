"""Per-frame image metrics of the reference's Evaluator (lib/evaluators/if_nerf.py) on the device: ctypes wrappers of
invr_image_assemble / invr_image_metrics (include/invr.h, csrc/k_metrics.hip).  Everything is enqueued on the current stream and
nothing is read back here: a frame's numbers stay in its 64-byte device result block until `decode()` is handed a host copy."""
import ctypes as C

import numpy as np
import torch

from . import _abi

RESULT_BYTES = _abi.EVAL_RESULT_BYTES
WINDOW = 7                                   # skimage's default win_size


def workspace_bytes(H, W):
    n = int(_abi.lib().invr_eval_workspace_bytes(int(H), int(W)))
    if n == 0:
        raise ValueError('invr_eval_workspace_bytes: unsupported image size %r x %r' % (H, W))
    return n


def new_workspace(H, W, device):
    """uint8 tensor of workspace_bytes(H, W) at a 256-byte aligned address on `device`."""
    n = workspace_bytes(H, W)
    raw = torch.empty(n + 256, dtype=torch.uint8, device=device)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + n]


def new_results(count, device):
    """(count, RESULT_BYTES) uint8: one result block per frame (8-byte aligned rows)."""
    return torch.zeros((int(count) * RESULT_BYTES // 8,), dtype=torch.int64, device=device).view(torch.uint8).view(int(count), RESULT_BYTES)


def _mask_u8(mask, device):
    mask = mask.reshape(-1)
    if mask.dtype == torch.bool:
        mask = mask.contiguous().view(torch.uint8)
    elif mask.dtype != torch.uint8:
        mask = (mask != 0).view(torch.uint8)
    return mask.to(device, non_blocking=True).contiguous()


def _values(t, device):
    return t.detach().reshape(-1, 3).to(device=device, dtype=torch.float32, non_blocking=True).contiguous()


def image_assemble(pred, gt, mask, H, W, result, workspace, want_u8=False):
    """img[mask] = values for the rendered and the ground-truth pixels (if_nerf.py:39-42, 85-89), cv2.boundingRect(mask) (:68)
    into `result`, and optionally the B,G,R uint8 images cv2.imwrite stores (:58-65).  pred, gt (n,3); mask (H*W) bool / uint8.
    -> (img_pred, img_gt, u8_pred, u8_gt), the u8 images None unless want_u8.  Tensors are allocated on result's device."""
    H, W = int(H), int(W)
    dev = result.device
    pred, gt, mask = _values(pred, dev), _values(gt, dev), _mask_u8(mask, dev)
    if pred.shape != gt.shape:
        raise ValueError('image_assemble: %d predicted rows, %d ground-truth rows' % (pred.shape[0], gt.shape[0]))
    if mask.numel() != H * W:
        raise ValueError('image_assemble: mask has %d entries, H * W = %d' % (mask.numel(), H * W))
    img_pred = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    img_gt = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    u8_pred = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    u8_gt = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    _abi.check(_abi.lib().invr_image_assemble(
        _abi.ptr(pred), _abi.ptr(gt), _abi.ptr(mask, torch.uint8), pred.shape[0], H, W, _abi.ptr(img_pred), _abi.ptr(img_gt),
        _abi.ptr(u8_pred, torch.uint8), _abi.ptr(u8_gt, torch.uint8), _abi.ptr(result, torch.uint8),
        _abi.ptr(workspace, torch.uint8), C.c_size_t(workspace.numel()), _abi.stream_ptr()))
    return img_pred, img_gt, u8_pred, u8_gt


def image_metrics(img_pred, img_gt, result, workspace, crop=False):
    """SSE, sum gt and the SSIM sums of two (H,W,3) float32 images into `result`; crop: SSIM over the rectangle image_assemble left
    there (cfg.test_full False, if_nerf.py:68-72) instead of the whole frame (:126)."""
    H, W = int(img_pred.shape[0]), int(img_pred.shape[1])
    if tuple(img_pred.shape) != (H, W, 3) or img_gt.shape != img_pred.shape:
        raise ValueError('image_metrics: two (H,W,3) images expected, got %r and %r' % (tuple(img_pred.shape), tuple(img_gt.shape)))
    _abi.check(_abi.lib().invr_image_metrics(
        _abi.ptr(img_pred), _abi.ptr(img_gt), H, W, int(bool(crop)), _abi.ptr(result, torch.uint8),
        _abi.ptr(workspace, torch.uint8), C.c_size_t(workspace.numel()), _abi.stream_ptr()))


def decode(block):
    """A HOST copy of one result block (RESULT_BYTES uint8: tensor, bytes or array) -> dict(sse, sum_gt, sum_s float64; windows, x,
    y, w, h, status, n_set int)."""
    raw = np.ascontiguousarray(block.numpy() if torch.is_tensor(block) else np.frombuffer(bytes(block), dtype=np.uint8))
    f = raw[:24].view(np.float64)
    i = raw[24:56].view(np.int32)
    return {'sse': f[0], 'sum_gt': f[1], 'sum_s': f[2], 'windows': int(i[0]), 'x': int(i[1]), 'y': int(i[2]), 'w': int(i[3]),
            'h': int(i[4]), 'status': int(i[5]), 'n_set': int(i[6])}


def mse_of(r, H, W, test_full=True):
    """np.mean((img_pred - img_gt) ** 2) of if_nerf.py:112 (whole frame) / :137 (the n rays inside the box)."""
    count = 3 * int(H) * int(W) if test_full else 3 * r['n_set']
    return r['sse'] / np.float64(count)


def psnr_of(mse):
    """Evaluator.psnr_metric (if_nerf.py:28-31), the reference's own expression in NumPy float64"""
    return -10 * np.log(mse) / np.log(10)


def ssim_of(r):
    if r['windows'] <= 0:
        raise ValueError('win_size exceeds image extent: the image%s has a side shorter than %d pixels'
                         % (' (%d x %d)' % (r['w'], r['h']) if r['w'] or r['h'] else '', WINDOW))
    return r['sum_s'] / np.float64(3 * r['windows'])
