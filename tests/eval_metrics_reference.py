"""TEST INFRASTRUCTURE — a float64 NumPy restatement of the per-frame image metrics of the reference's Evaluator
(lib/evaluators/if_nerf.py with scikit-image 0.19.3 and OpenCV 4.7), written from their definitions: neither package is part of this
project's environment.  The device kernels (instant-nvr_amd/csrc/k_metrics.hip) are tested against THIS, never against themselves.

  assemble        img = zeros((H,W,3)); img[mask] = values                                      (:39-42, :85-89)
  bounding_rect   cv2.boundingRect(mask): x, y = smallest column / row with a set pixel, w, h = largest - smallest + 1; zeros when empty (:68)
  ssim            skimage.metrics.structural_similarity(a, b, channel_axis=2) on float64 images, defaults: uniform 7x7 window, K1 0.01,
                  K2 0.03, sample covariance (cov_norm 49/48), data_range 2 (dtype_range[float64] = (-1, 1)); the library crops 3 pixels
                  from every border before it averages, so the result is the mean of S over the windows that lie fully inside the image
  to_u8_bgr       cv2.imwrite(img[..., [2,1,0]] * 255): saturate_cast<uchar>(double) = round half to even, clamp to 0..255 (from
                  OpenCV's documentation)
"""
import numpy as np

WIN = 7
K1, K2, DATA_RANGE = 0.01, 0.03, 2.0
C1, C2 = (K1 * DATA_RANGE) ** 2, (K2 * DATA_RANGE) ** 2
COV_NORM = WIN * WIN / (WIN * WIN - 1.0)


def assemble(values, mask, H, W, dtype=np.float64):
    img = np.zeros((H, W, 3), dtype=dtype)
    img[np.asarray(mask, dtype=bool).reshape(H, W)] = values
    return img


def bounding_rect(mask, H, W):
    m = np.asarray(mask, dtype=bool).reshape(H, W)
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def _window_means(a):
    """mean over every 7x7 window fully inside the (h,w) float64 image -> (h-6, w-6)"""
    h, w = a.shape
    out = np.zeros((h - WIN + 1, w - WIN + 1), dtype=np.float64)
    for dy in range(WIN):
        for dx in range(WIN):
            out += a[dy:dy + h - WIN + 1, dx:dx + w - WIN + 1]
    return out / (WIN * WIN)


def ssim_channel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ux, uy = _window_means(a), _window_means(b)
    uxx, uyy, uxy = _window_means(a * a), _window_means(b * b), _window_means(a * b)
    vx, vy, vxy = COV_NORM * (uxx - ux * ux), COV_NORM * (uyy - uy * uy), COV_NORM * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean(dtype=np.float64)


def ssim(img_a, img_b):
    """-> float64; ValueError when a side is shorter than the window (as scikit-image raises)"""
    if min(img_a.shape[0], img_a.shape[1]) < WIN:
        raise ValueError('win_size exceeds image extent')
    return np.mean([ssim_channel(img_a[..., c], img_b[..., c]) for c in range(3)], dtype=np.float64)


def to_u8_bgr(img):
    v = np.rint(np.asarray(img, dtype=np.float64)[..., [2, 1, 0]] * 255.0)          # np.rint: round half to even
    return np.clip(v, 0, 255).astype(np.uint8)


def psnr(mse):
    return -10 * np.log(mse) / np.log(10)


def frame_metrics(pred, gt, mask, H, W, test_full=True):
    """Everything the tests compare, for one frame: pred, gt (n,3) float32, mask (H*W).  -> dict"""
    pred32, gt32 = np.asarray(pred, dtype=np.float32).reshape(-1, 3), np.asarray(gt, dtype=np.float32).reshape(-1, 3)
    img_p, img_g = assemble(pred32, mask, H, W), assemble(gt32, mask, H, W)
    x, y, w, h = bounding_rect(mask, H, W)
    n = pred32.shape[0]
    sse = np.sum((img_p - img_g) ** 2, dtype=np.float64)
    out = {'img_pred': img_p.astype(np.float32), 'img_gt': img_g.astype(np.float32), 'rect': (x, y, w, h), 'sse': sse,
           'sum_gt': np.sum(img_g, dtype=np.float64), 'u8_pred': to_u8_bgr(img_p), 'u8_gt': to_u8_bgr(img_g), 'n': n}
    if test_full:
        a, b, count = img_p, img_g, 3 * H * W
    else:
        a, b, count = img_p[y:y + h, x:x + w], img_g[y:y + h, x:x + w], 3 * n
    out['mse'] = sse / np.float64(count) if count else np.float64('nan')
    out['windows'] = (a.shape[0] - 6) * (a.shape[1] - 6) if min(a.shape[0], a.shape[1]) >= WIN else 0
    out['ssim'] = ssim(a, b) if out['windows'] else None
    return out
