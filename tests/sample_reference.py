"""NumPy restatement (checker only) of the plain N_rand sampling path: the reference's sample_ray_h36m
(lib/utils/if_nerf/if_nerf_data_utils.py:228-297 with get_rays :24-38, get_near_far :92-107, get_bound_2d_mask :78-89) as
invr.trainset / invr.raysample / include/invr_sample.h split it.  Written from those rules in the straightforward way — whole
coordinate lists from np.argwhere, whole-frame ray arrays — and sharing no code with the product:

  hull_mask    the closed convex hull of integer points by brute force over pixels, Python-int cross products, no hull algorithm
  classes      the three pixel classes as np.argwhere coordinate lists
  draw_rays    the sampling loop on those lists -> (class, rank) rows and the per-round structure
  ray_batch    the contract of include/invr_sample.h, following the reference's expressions line for line
  plain_batch  the whole item of tpose_dataset.py:442-450 for one frame under a seed

tests/golden/sample_small.npz holds the reference's own outputs for them to be held against."""
import functools
import os

import numpy as np

f32, f64 = np.float32, np.float64


# ---- the bound mask -------------------------------------------------------------------------------------------------------------------
def corners_2d(wbounds, K, R, T):
    """get_bound_corners + base_utils.project + np.round(...).astype(int) -> (8,2) ints (x, y), and the corners' depths."""
    bounds = np.asarray(wbounds, f32).reshape(2, 3)
    min_x, min_y, min_z = bounds[0]
    max_x, max_y, max_z = bounds[1]
    corners_3d = np.array([[min_x, min_y, min_z], [min_x, min_y, max_z], [min_x, max_y, min_z], [min_x, max_y, max_z],
                           [max_x, min_y, min_z], [max_x, min_y, max_z], [max_x, max_y, min_z], [max_x, max_y, max_z]])
    RT = np.concatenate([np.asarray(R, f64).reshape(3, 3), np.asarray(T, f64).reshape(3, 1)], axis=1)
    xyz = np.dot(corners_3d, RT[:, :3].T) + RT[:, 3:].T
    depth = xyz[:, 2].copy()
    xyz = np.dot(xyz, np.asarray(K, f64).reshape(3, 3).T)
    return np.round(xyz[:, :2] / xyz[:, 2:]).astype(int), depth


def hull_mask(pts, H, W):
    """(H,W) uint8: 1 where the pixel lies in the closed convex hull of the integer points.  Brute force: a pixel is in the hull iff it
    is within the points' bounding box and on the left of, or on, every directed line through two distinct points that has ALL the
    points on its left or on it (the supporting lines; collinear points give both directions, i.e. the line itself)."""
    pts = [(int(x), int(y)) for x, y in np.asarray(pts).reshape(-1, 2)]
    cross = lambda a, b, p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])
    lines = [(a, b) for a in pts for b in pts if a != b and all(cross(a, b, q) >= 0 for q in pts)]
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    mask = np.zeros((H, W), np.uint8)
    for y in range(max(min(ys), 0), min(max(ys), H - 1) + 1):
        for x in range(max(min(xs), 0), min(max(xs), W - 1) + 1):
            mask[y, x] = all(cross(a, b, (x, y)) >= 0 for a, b in lines)
    return mask


@functools.lru_cache(maxsize=None)
def _bound_mask(wb, K, R, T, H, W):
    pts, depth = corners_2d(np.frombuffer(wb, f32), np.frombuffer(K, f64), np.frombuffer(R, f64), np.frombuffer(T, f64))
    assert (depth > 0).all()
    return hull_mask(pts, H, W)


def bound_mask(wbounds, K, R, T, H, W):
    """The default bound mask of a frame (cached per camera and box; treat as read-only)."""
    c = lambda a, t: np.ascontiguousarray(a, t).tobytes()
    return _bound_mask(c(wbounds, f32), c(K, f64), c(R, f64), c(T, f64), H, W)


# ---- classes and the draw ---------------------------------------------------------------------------------------------------------------
def classes(msk, bound, face_value=13):
    """-> [coord_body, coord_face, coord_bound]: (len,2) (row, col) lists in np.argwhere order, after msk = msk * bound_mask and
    bound_mask[msk == 100] = 0 (:238-239)."""
    bound = np.array(bound, np.uint8)
    msk = np.asarray(msk, np.uint8) * bound
    bound[msk == 100] = 0
    return [np.argwhere(msk == 1), np.argwhere(msk == face_value), np.argwhere(bound == 1)]


def frame_rays(H, W, K, R, T):
    """get_rays -> rays_o (3,), rays_d (H,W,3), float64."""
    K, R, T = np.asarray(K, f64).reshape(3, 3), np.asarray(R, f64).reshape(3, 3), np.asarray(T, f64).reshape(3, 1)
    rays_o = -np.dot(R.T, T).ravel()
    i, j = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32), indexing='xy')
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = np.dot(xy1, np.linalg.inv(K).T)
    pixel_world = np.dot(pixel_camera - T.ravel(), R)
    rays_d = pixel_world - rays_o[None, None]
    rays_d = rays_d / np.linalg.norm(rays_d, axis=2, keepdims=True)
    return rays_o, rays_d


def near_far(bounds, ray_o, ray_d):
    """get_near_far on (n,3) float64 rays -> near, far (all n, float64, already divided by norm_d) and mask_at_box."""
    bounds = np.asarray(bounds, f32).reshape(2, 3)
    norm_d = np.linalg.norm(ray_d, axis=-1, keepdims=True)
    viewdir = ray_d / norm_d
    viewdir[(viewdir < 1e-5) & (viewdir > -1e-10)] = 1e-5
    viewdir[(viewdir > -1e-5) & (viewdir < 1e-10)] = -1e-5
    tmin = (bounds[:1] - ray_o[None]) / viewdir
    tmax = (bounds[1:2] - ray_o[None]) / viewdir
    near = np.max(np.minimum(tmin, tmax), axis=-1)
    far = np.min(np.maximum(tmin, tmax), axis=-1)
    return near / norm_d[:, 0], far / norm_d[:, 0], near < far


def draw_rays(coords, inside, n_rays, body_ratio, face_ratio, rng=None):
    """The `while nsampled_rays < nrays` loop (:253-289).  coords: the three lists of `classes`; inside (H,W) bool: mask_at_box of every
    pixel.  -> sel (n,2) int32 (class, rank), and per round (n_body, n_face drawn or -1 when the face class is empty, n_rand, kept)."""
    rng = np.random if rng is None else rng
    coord_body_all, coord_face_all, coord_all = coords
    sel, rounds, nsampled_rays = [], [], 0
    while nsampled_rays < n_rays:
        n_body = int((n_rays - nsampled_rays) * body_ratio)
        n_face = int((n_rays - nsampled_rays) * face_ratio)
        n_rand = (n_rays - nsampled_rays) - n_body - n_face
        drawn = [(0, rng.randint(0, len(coord_body_all), n_body))]
        if len(coord_face_all) > 0:
            drawn.append((1, rng.randint(0, len(coord_face_all), n_face)))
        drawn.append((2, rng.randint(0, len(coord_all), n_rand)))
        cls = np.concatenate([np.full(len(r), c) for c, r in drawn])
        rank = np.concatenate([r for _, r in drawn])
        coord = np.concatenate([coords[c][r] for c, r in drawn], axis=0)
        mask_at_box = inside[coord[:, 0], coord[:, 1]]
        sel.append(np.stack([cls[mask_at_box], rank[mask_at_box]], 1))
        nsampled_rays += int(mask_at_box.sum())
        rounds.append((n_body, n_face if len(coord_face_all) > 0 else -1, n_rand, int(mask_at_box.sum())))
    return np.concatenate(sel).astype(np.int32), rounds


# ---- the contract of include/invr_sample.h ----------------------------------------------------------------------------------------------
def planes_and_prefix(coords, H, W):
    """The device form of the three classes, built pixel by pixel from the coordinate lists: planes (3,H,ceil(W/64)) uint64 and
    row_prefix (3,H+1) int32."""
    wr = (W + 63) // 64
    planes, prefix = np.zeros((3, H, wr), np.uint64), np.zeros((3, H + 1), np.int32)
    for c, co in enumerate(coords):
        for y, x in co:
            planes[c, y, x // 64] |= np.uint64(1) << np.uint64(x % 64)
        prefix[c, 1:] = np.cumsum(np.bincount(co[:, 0], minlength=H)) if len(co) else 0
    return planes, prefix


def ray_batch(img, occ_msk, coords, sel, K, R, T, bounds):
    """The rows invr_ray_batch writes for `sel` -> dict(ray_d, near, far, rgb, occupancy, coord).  The pixel of a row is
    coords[class][rank]; its ray follows get_rays with the sums written out left to right, its near / far follow get_near_far in float64."""
    H, W = np.asarray(occ_msk).shape
    K, R, T = np.asarray(K, f64).reshape(3, 3), np.asarray(R, f64).reshape(3, 3), np.asarray(T, f64).reshape(3)
    k = np.linalg.inv(K)
    o = -np.dot(R.T, T.reshape(3, 1)).ravel()
    sel = np.asarray(sel)
    coord = np.zeros((len(sel), 2), np.int64)
    for c in range(3):
        coord[sel[:, 0] == c] = coords[c][sel[sel[:, 0] == c, 1]].reshape(-1, 2)
    i, j = coord[:, 1].astype(f32).astype(f64), coord[:, 0].astype(f32).astype(f64)
    pc = np.stack([(i * k[a, 0] + j * k[a, 1]) + k[a, 2] for a in range(3)], 1)
    q = pc - T
    pw = np.stack([q[:, 0] * R[0, b] + q[:, 1] * R[1, b] + q[:, 2] * R[2, b] for b in range(3)], 1)
    d = pw - o
    d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
    with np.errstate(divide='ignore', invalid='ignore'):
        near, far, _ = near_far(bounds, o, d)
    return {'ray_d': d.astype(f32), 'near': near.astype(f32), 'far': far.astype(f32), 'rgb': np.asarray(img)[coord[:, 0], coord[:, 1]],
            'occupancy': np.asarray(occ_msk)[coord[:, 0], coord[:, 1]], 'coord': coord}


def plain_batch(img, msk, orig_msk, K, R, T, wbounds, n_rays, body_ratio, face_ratio, rng=None, bound=None, face_value=13):
    """The ray part of the reference item (tpose_dataset.py:442-463) of one frame, un-collated: rgb, occupancy, coord, ray_o, ray_d,
    near, far, mask_at_box; plus `sel` and `rounds` of the draw."""
    H, W = np.asarray(msk).shape
    bound = bound_mask(wbounds, K, R, T, H, W) if bound is None else bound
    coords = classes(msk, bound, face_value)
    rays_o, rays_d = frame_rays(H, W, K, R, T)
    inside = near_far(wbounds, rays_o, rays_d.reshape(-1, 3))[2].reshape(H, W)
    sel, rounds = draw_rays(coords, inside, n_rays, body_ratio, face_ratio, rng)
    r = ray_batch(img, orig_msk, coords, sel, K, R, T, wbounds)
    n = len(sel)
    r.update(ray_o=np.broadcast_to(rays_o.astype(f32), (n, 3)), mask_at_box=np.ones(n, bool), sel=sel, rounds=rounds)
    return r


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def synthetic_orig_msk(msk, face=None):
    """The occupancy mask of the fixtures: 1 where the frame's mask is set (its ring of 100 included), 7 there on every fifth row — so
    that occupancy is seen to be the BYTE of orig_msk, not a flag and not `msk`."""
    o = (np.asarray(msk) > 0).astype(np.uint8)
    o[::5] *= 7
    return o


def with_face(msk, H, W):
    """A copy of a fixture mask with a face: the value 13 in a small disc in the upper part of the body."""
    yy, xx = np.mgrid[0:H, 0:W]
    m = np.array(msk)
    m[((xx - W / 2.0) ** 2 + (yy - 0.3 * H) ** 2 <= (0.06 * min(H, W)) ** 2) & (m == 1)] = 13
    return m


_GOLDEN = None


def golden_cases():
    """tests/golden/sample_small.npz (tests/golden/make_golden_sample.py: the imported reference's own sample_ray_h36m) -> a list of
    cases: the frame (img, msk, orig_msk, K, R, T, wbounds, bound), the draw's inputs (seed, N_rand, body_ratio, face_ratio) and the
    reference's results (coord, occupancy, ray_d, near, far, rounds), with `ulp` = the bound the golden's metadata records for
    ray_d / near / far (0: bit for bit).  Loaded once; treat as read-only."""
    global _GOLDEN
    if _GOLDEN is None:
        from tests import patch_reference as P
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sample_small.npz'))
        frames, cases = {}, []
        for name in g['cases']:
            tag = str(g[name + '_scene'])
            if tag not in frames:
                H, W, img_seed, face = (int(v) for v in g[tag + '_meta'])
                msk, _ = P.synthetic_masks(H, W)
                if face:
                    msk = with_face(msk, H, W)
                frames[tag] = dict(H=H, W=W, msk=msk, orig_msk=synthetic_orig_msk(msk), img=P.synthetic_image(H, W, img_seed, msk), K=g[tag + '_K'],
                                   R=g[tag + '_R'], T=g[tag + '_T'], wbounds=g[tag + '_wbounds'],
                                   bound=np.unpackbits(g[tag + '_bound'])[:H * W].reshape(H, W))
            seed, n_rand = (int(v) for v in g[name + '_draw'])
            body_ratio, face_ratio = (float(v) for v in g[name + '_ratios'])
            c = dict(frames[tag], name=str(name), scene=tag, seed=seed, N_rand=n_rand, body_ratio=body_ratio, face_ratio=face_ratio,
                     ulp=int(g['max_ulp']), rounds=[tuple(int(v) for v in r) for r in g[name + '_rounds']])
            for k in ('coord', 'occupancy', 'ray_d', 'near', 'far'):
                c[k] = g[name + '_' + k]
            cases.append(c)
        _GOLDEN = cases
    return _GOLDEN


def ulp_distance(a, b):
    """Largest distance in float32 units in the last place between two float32 arrays of finite values."""
    def key(x):
        i = np.ascontiguousarray(x, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max()) if np.size(a) else 0
