"""Host side of the plain N_rand sampling of invr.trainset (the reference's sample_ray_h36m, lib/utils/if_nerf/if_nerf_data_utils.py
:228-297): everything that is fixed per frame, computed once when the frame is added, and the draw loop that then needs no device result.

  bound_mask      get_bound_2d_mask (:78-89) without cv2: the closed convex hull of the eight rounded box corners, in integer arithmetic.
  frame_classes   the three pixel classes a ray is drawn from (body, face, bound), each as row prefix counts + a bit plane for the
                  kernel (include/invr_sample.h) and, per member in row-major order, the reference's own mask_at_box decision.
  draw_rays       the `while nsampled_rays < nrays` loop (:253-289) with the reference's randint calls in its order -> (class, rank) rows.
"""
import numpy as np

BODY, FACE, BOUND = 0, 1, 2
CLASS_NAMES = ('body', 'face', 'bound')


def bound_corners(wbounds, K, R, T):
    """The eight corners of the box projected and rounded as get_bound_2d_mask does (get_bound_corners :62-75, base_utils.project,
    np.round(...).astype(int)) -> (8,2) int64 (x, y).  Raises if a corner is not in front of the camera: the hull of the projected corners
    is the box's silhouette only when all of them are."""
    b = np.asarray(wbounds, np.float32).reshape(2, 3)
    (x0, y0, z0), (x1, y1, z1) = b
    corners = np.array([[x0, y0, z0], [x0, y0, z1], [x0, y1, z0], [x0, y1, z1], [x1, y0, z0], [x1, y0, z1], [x1, y1, z0], [x1, y1, z1]])
    K, R, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 1)
    cam = np.dot(corners, R.T) + T.T
    if not (cam[:, 2] > 0).all():
        raise ValueError('bound_mask: a corner of the box has depth %.6g <= 0: it is not in front of the camera' % cam[:, 2].min())
    xyz = np.dot(cam, K.T)
    return np.round(xyz[:, :2] / xyz[:, 2:]).astype(np.int64)


def convex_hull(pts):
    """Andrew's monotone chain on integer points -> the hull's vertices counter-clockwise in (x, y) axes, collinear points dropped
    (one vertex for coincident points, two for collinear ones).  Python integers: exact."""
    p = sorted(set((int(x), int(y)) for x, y in pts))
    if len(p) <= 2:
        return p
    cross = lambda o, a, b: (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])
    lower, upper = [], []
    for q in p:
        while len(lower) >= 2 and cross(lower[-2], lower[-1], q) <= 0:
            lower.pop()
        lower.append(q)
    for q in reversed(p):
        while len(upper) >= 2 and cross(upper[-2], upper[-1], q) <= 0:
            upper.pop()
        upper.append(q)
    return lower[:-1] + upper[:-1]


def hull_mask(pts, H, W):
    """(H,W) uint8: pixel (x, y) is 1 iff it lies on or inside every edge of the convex hull of the integer points `pts` (closed hull:
    vertices and edges belong to it; a degenerate hull is its segment or its single pixel)."""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    if np.abs(pts).max() >= 2 ** 29:
        raise ValueError('hull_mask: a projected corner lies %d pixels out: beyond exact 64-bit arithmetic' % np.abs(pts).max())
    mask = np.zeros((H, W), np.uint8)
    x_lo, y_lo = max(int(pts[:, 0].min()), 0), max(int(pts[:, 1].min()), 0)
    x_hi, y_hi = min(int(pts[:, 0].max()), W - 1), min(int(pts[:, 1].max()), H - 1)
    if x_lo > x_hi or y_lo > y_hi:
        return mask
    hull = convex_hull(pts)
    yy, xx = np.mgrid[y_lo:y_hi + 1, x_lo:x_hi + 1].astype(np.int64)
    inside = np.ones(xx.shape, bool)                                   # the points' bounding box: all of a one-pixel hull, the ends of a segment
    if len(hull) >= 2:
        for (ax, ay), (bx, by) in zip(hull, hull[1:] + hull[:1]):       # a segment is walked both ways: cross == 0
            inside &= (bx - ax) * (yy - ay) - (by - ay) * (xx - ax) >= 0
    mask[y_lo:y_hi + 1, x_lo:x_hi + 1] = inside
    return mask


def bound_mask(wbounds, K, R, T, H, W):
    """get_bound_2d_mask without cv2: the union of the six face polygons it fills is the hull of the eight corners.  May differ from
    cv2.fillPoly on pixels of the hull's outline only (cv2 also draws the outline with its line iterator)."""
    return hull_mask(bound_corners(wbounds, K, R, T), H, W)


def inside_box(H, W, K, R, T, wbounds):
    """(H,W) bool: mask_at_box of every pixel as sample_ray_h36m decides it — get_rays (:24-38) then get_near_far (:92-107) on the
    float64 rays and the float64 camera centre, bounds float32, evaluated over the frame with the reference's own NumPy expressions."""
    K, R, T = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(T, np.float64).reshape(3, 1)
    bounds = np.asarray(wbounds, np.float32).reshape(2, 3)
    rays_o = -np.dot(R.T, T).ravel()
    i, j = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32), indexing='xy')
    xy1 = np.stack([i, j, np.ones_like(i)], axis=2)
    pixel_camera = np.dot(xy1, np.linalg.inv(K).T)
    pixel_world = np.dot(pixel_camera - T.ravel(), R)
    rays_d = pixel_world - rays_o[None, None]
    rays_d = rays_d / np.linalg.norm(rays_d, axis=2, keepdims=True)
    ray_d = rays_d.reshape(-1, 3)
    norm_d = np.linalg.norm(ray_d, axis=-1, keepdims=True)
    viewdir = ray_d / norm_d
    viewdir[(viewdir < 1e-5) & (viewdir > -1e-10)] = 1e-5
    viewdir[(viewdir > -1e-5) & (viewdir < 1e-10)] = -1e-5
    tmin = (bounds[:1] - rays_o[None]) / viewdir
    tmax = (bounds[1:2] - rays_o[None]) / viewdir
    near = np.max(np.minimum(tmin, tmax), axis=-1)
    far = np.min(np.maximum(tmin, tmax), axis=-1)
    return (near < far).reshape(H, W)


class FrameClasses:
    """The pixel classes of one frame.  sizes (3,); inside[c] bool per rank (host only); row_prefix (3, H+1) int32 and planes
    (3, H, ceil(W/64)) uint64 for the device."""

    def __init__(self, msk, bound, inside, face_value=13):
        H, W = msk.shape
        bound = np.array(bound, np.uint8)                               # a copy: zeroed below
        m = msk * bound                                                 # :238
        bound[m == 100] = 0                                             # :239
        members = [m == 1, m == face_value, bound == 1]                  # :259, :263, :268
        wr = (W + 63) // 64
        self.sizes = np.array([int(c.sum()) for c in members], np.int64)
        self.inside = [np.ascontiguousarray(inside[c]) for c in members]            # boolean indexing runs in np.argwhere's order
        self.row_prefix = np.zeros((3, H + 1), np.int32)
        self.planes = np.zeros((3, H, wr), np.uint64)
        for c, member in enumerate(members):
            self.row_prefix[c, 1:] = np.cumsum(member.sum(1, dtype=np.int64))
            padded = np.zeros((H, wr * 64), np.uint8)
            padded[:, :W] = member
            self.planes[c] = np.packbits(padded, axis=1, bitorder='little').view('<u8')


def draw_rays(classes, n_rays, body_ratio, face_ratio, rng=None, frame='?'):
    """The reference's sampling loop on the classes of one frame -> sel (n,2) int32 (class, rank), n >= n_rays: per round
    randint(0, len_body, n_body), then — only if the face class has members — randint(0, len_face, n_face), then
    randint(0, len_bound, n_rand); the round keeps the draws whose ray meets the box, in that order."""
    rng = np.random if rng is None else rng
    n_rays = int(n_rays)
    len_body, len_face, len_bound = (int(v) for v in classes.sizes)
    if len_body == 0:
        raise ValueError('draw_rays: frame %s has no body pixel inside its bound mask (the reference\'s randint(0, 0, n) raises there)' % (frame,))
    if not any(classes.inside[c].any() for c in (BODY, BOUND)):
        raise ValueError('draw_rays: no body or bound pixel of frame %s has a ray that meets the box: the loop would never end' % (frame,))
    rounds, sampled = [], 0
    while sampled < n_rays:
        rem = n_rays - sampled
        n_body = int(rem * body_ratio)
        n_face = int(rem * face_ratio)
        n_rand = rem - n_body - n_face
        parts = [(BODY, rng.randint(0, len_body, n_body))]
        if len_face > 0:
            parts.append((FACE, rng.randint(0, len_face, n_face)))
        parts.append((BOUND, rng.randint(0, len_bound, n_rand)))
        for c, ranks in parts:
            kept = ranks[classes.inside[c][ranks]]
            rounds.append(np.stack([np.full(len(kept), c, np.int64), kept.astype(np.int64)], 1))
            sampled += len(kept)
    return np.ascontiguousarray(np.concatenate(rounds).astype(np.int32))
