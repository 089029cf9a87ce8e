"""NumPy restatement (checker only) of the training-patch path: the contract of include/invr_batch.h (`patch_batch`) and the host-side
window draw of invr.trainset.TrainSet.draw (`draw`), i.e. the patch branch of the reference's dataset
(lib/datasets/h36m/tpose_dataset.py:421-441 -> lib/utils/if_nerf/if_nerf_data_utils.py: crop_image_msk :611-643, padding_bbox
:580-608, random_crop_image :647-686, get_rays_within_bounds_coord :329-343).  Written from those rules, in the straightforward way:
whole coordinate lists, whole-window arrays.  tests/golden/patch_small.npz holds the reference's own outputs for it to be held against."""
import numpy as np

f32, f64 = np.float32, np.float64


def bounding_rect(mask):
    """cv2.boundingRect of a single-channel mask: (x, y, w, h) of the non-zero pixels, (0, 0, 0, 0) when there are none."""
    ys, xs = np.nonzero(np.asarray(mask))
    if len(ys) == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def crop_rect(ref_msk, H, W, patch_size):
    """crop_image_msk's rectangle [[x_lo, y_lo], [x_hi, y_hi]] (hi exclusive) around the non-zero pixels of ref_msk in an H x W frame, or
    None when their bounding rectangle is narrower or lower than a patch."""
    x, y, w, h = bounding_rect(ref_msk)
    if w < patch_size or h < patch_size:
        return None
    b = np.array([[x - 10, y - 10], [x + w + 10, y + h + 10]], dtype=np.int64)
    height, width = int(b[1, 1] - b[0, 1]), int(b[1, 0] - b[0, 0])
    if height / width > 1.5:
        m = int(height / 1.5)
        if width < m:
            b[0, 0] -= (m - width) // 2
            b[1, 0] += (m - width) // 2
    if width / height > 1.5:
        m = int(width / 1.5)
        if height < m:
            b[0, 1] -= (m - height) // 2
            b[1, 1] += (m - height) // 2
    b[:, 0] = np.clip(b[:, 0], 0, W - 1)
    b[:, 1] = np.clip(b[:, 1], 0, H - 1)
    return b


def draw(msk, ref_msk, K, patch_size, rng=None):
    """-> (x0, y0, w, h, K32): the window in frame coordinates and its float32 intrinsic matrix.  msk (H, W) with values 0 / 1 / 100;
    ref_msk the mask the crop rectangle is taken from (msk itself, or the focused semantic mask); K (3,3) float64.  Draws from rng
    (a RandomState; None = the global np.random) in the reference's order: the side, then the centre pixel."""
    rng = np.random if rng is None else rng
    H, W = msk.shape
    b = crop_rect(ref_msk, H, W, patch_size)
    K = np.array(K, dtype=f64)
    bx, by = 0, 0
    if b is not None:
        bx, by = int(b[0, 0]), int(b[0, 1])
        msk = msk[b[0, 1]:b[1, 1], b[0, 0]:b[1, 0]]
        K[0, 2] -= bx
        K[1, 2] -= by
        K = K.astype(f32)
    H, W = msk.shape
    m = min(H, W, patch_size)
    size = (int(rng.randint(int(min(patch_size, 0.8 * m)), m)) | 7) + 1
    if size > H or size > W:
        raise ValueError('a %d x %d window does not fit the %d x %d crop' % (size, size, W, H))
    coord = np.argwhere(msk == 1)
    cy, cx = (int(v) for v in coord[rng.randint(0, len(coord))])
    x, y = cx - size // 2, cy - size // 2
    x = 0 if x < 0 else x
    x = W - size if x + size > W else x
    y = 0 if y < 0 else y
    y = H - size if y + size > H else y
    K = K.copy()
    K[0, 2] = K[0, 2] - x                 # (a float32 entry minus an integer is formed in float64 and rounded on assignment)
    K[1, 2] = K[1, 2] - y
    return bx + x, by + y, size, size, K.astype(f32)


def camera(K32, R, T):
    """-> (k_inv float32 (3,3), R, T (3,), cam_o (3,)) as invr_patch_batch takes them."""
    R, T = np.asarray(R, f64), np.asarray(T, f64)
    return np.linalg.inv(np.asarray(K32, f32)), R, T.ravel(), -np.dot(R.T, T.reshape(3, 1)).ravel()


def patch_batch(img, msk, x0, y0, w, h, k_inv, R, T, cam_o, bounds):
    """The contract of include/invr_batch.h -> dict(ray_d, near, far, rgb, occupancy, coord, mask_at_box, count); the compact arrays
    hold `count` rows."""
    k = np.asarray(k_inv, f32).reshape(3, 3)
    R, T, o = np.asarray(R, f64).reshape(3, 3), np.asarray(T, f64).reshape(3), np.asarray(cam_o, f64).reshape(3)
    bounds = np.asarray(bounds, f32).reshape(2, 3)
    y, x = np.divmod(np.arange(w * h), w)
    i, j = x.astype(f32), y.astype(f32)
    pc = np.stack([(i * k[a, 0] + j * k[a, 1]) + k[a, 2] for a in range(3)], 1)
    assert pc.dtype == f32
    q = pc.astype(f64) - T
    pw = np.stack([q[:, 0] * R[0, b] + q[:, 1] * R[1, b] + q[:, 2] * R[2, b] for b in range(3)], 1)
    d = pw - o
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    rd, ro = d.astype(f32), o.astype(f32)
    norm = np.sqrt(rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1] + rd[:, 2] * rd[:, 2])
    v = rd / norm[:, None]
    v[(v < f32(1e-5)) & (v > f32(-1e-10))] = f32(1e-5)
    v[(v > f32(-1e-5)) & (v < f32(1e-10))] = f32(-1e-5)
    with np.errstate(divide='ignore', invalid='ignore'):
        t0, t1 = (bounds[0] - ro) / v, (bounds[1] - ro) / v
        near, far = np.minimum(t0, t1).max(1), np.maximum(t0, t1).min(1)
        inside = near < far
        near, far = near / norm, far / norm
    assert near.dtype == f32 and far.dtype == f32
    fy, fx = y0 + y[inside], x0 + x[inside]
    return {'ray_d': rd[inside], 'near': near[inside], 'far': far[inside], 'rgb': np.asarray(img)[fy, fx],
            'occupancy': (np.asarray(msk)[fy, fx] > 0).astype(np.uint8), 'coord': np.stack([x[inside], y[inside]], 1).astype(np.uint8),
            'mask_at_box': inside.astype(np.uint8), 'count': int(inside.sum())}


def synthetic_masks(H, W, cx=None, cy=None, ax=None, ay=None):
    """The masks of the patch fixtures: an ellipse of 1 with a ring of 100 around it (the reference's eroded / dilated border) in an
    H x W frame, and five semantic masks in PART_NAMES order of which only 'head' (index 2) is set: the ellipse's top quarter."""
    cx, cy = (W / 2.0 if cx is None else cx), (H / 2.0 if cy is None else cy)
    ax, ay = (0.36 * W if ax is None else ax), (0.44 * H if ay is None else ay)
    yy, xx = np.mgrid[0:H, 0:W]
    r = ((xx - cx) / ax) ** 2 + ((yy - cy) / ay) ** 2
    msk = np.zeros((H, W), np.uint8)
    msk[r <= 1.0] = 1
    msk[(r > 0.82) & (r <= 1.0)] = 100
    sem = np.zeros((5, H, W), np.uint8)
    sem[2] = ((msk > 0) & (yy < cy - ay / 2.0)).astype(np.uint8)
    return msk, sem


def synthetic_image(H, W, seed, msk):
    """The frame's pixels: uniform noise from the seed, zero outside the mask (cfg.mask_bkgd)."""
    img = np.random.RandomState(seed).rand(H, W, 3).astype(f32)
    img[msk == 0] = 0
    return img


PART_NAMES = ('body', 'leg', 'head', 'larm', 'rarm')
_GOLDEN = None


def golden_cases():
    """tests/golden/patch_small.npz (tests/golden/make_golden_patch.py: the imported reference's own outputs) -> a list of cases, each a
    dict with the frame (img, msk, sem, K, R, T, wbounds, patch_size), the draw's inputs (seed, focus) and the reference's results (window,
    K32, ray_d, near, far, coord, mask_at_box, occupancy).  Loaded once; treat as read-only."""
    global _GOLDEN
    if _GOLDEN is None:
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'patch_small.npz'))
        frames, cases = {}, []
        for name in g['cases']:
            tag, seed, fi, cropped = (int(v) for v in g[name + '_case'])
            tag = chr(tag)
            if tag not in frames:
                H, W, patch, img_seed = (int(v) for v in g[tag + '_meta'])
                msk, sem = synthetic_masks(H, W)
                frames[tag] = dict(H=H, W=W, patch_size=patch, msk=msk, sem=sem, img=synthetic_image(H, W, img_seed, msk), K=g[tag + '_K'],
                                   R=g[tag + '_R'], T=g[tag + '_T'], wbounds=g[tag + '_wbounds'])
            c = dict(frames[tag], name=str(name), scene=tag, seed=seed, focus=PART_NAMES[fi] if fi >= 0 else '', cropped=bool(cropped))
            x0, y0, w, h = (int(v) for v in g[name + '_window'])
            c.update(window=(x0, y0, w, h), K32=g[name + '_K32'], ray_d=g[name + '_ray_d'], near=g[name + '_near'], far=g[name + '_far'],
                     coord=g[name + '_coord'], mask_at_box=np.unpackbits(g[name + '_mask_at_box'])[:w * h])
            c['occupancy'] = np.unpackbits(g[name + '_occupancy'])[:len(c['near'])]
            cases.append(c)
        _GOLDEN = cases
    return _GOLDEN


def ref_mask(case):
    """The mask the crop rectangle of a golden case is taken from (tpose_dataset.py:424): msk, unless a non-empty focus mask is set."""
    if case['focus'] == '':
        return case['msk']
    sm = case['sem'][PART_NAMES.index(case['focus'])]
    return sm if sm.sum() != 0 else case['msk']
