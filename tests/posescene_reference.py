"""CHECKER ONLY — NumPy float64 restatement of include/invr_posescene.h's contract and of the few reference lines a posed frame's
scene tensors come from.  psbody.mesh / CGAL (tools/prepare_zjumocap.py:459-499, get_bweights) are not available, so the distance
volume's reference is the contract's brute force itself, chunked over the lattice points.

Cited lines of the reference:
  tools/prepare_zjumocap.py:152-165        get_grid_points: float64 min / max of the vertices -+ 0.05, np.arange with 0.025 per axis
  lib/utils/if_nerf/if_nerf_data_utils.py:689-696   get_bounds: min / max -+ cfg.box_padding, then astype(float32)
  lib/datasets/h36m/tpose_dataset.py:270   pxyz = np.dot(wxyz - Th, R).astype(np.float32)
  lib/datasets/h36m/tpose_dataset.py:570-600   the per-part reference sets and their trimmed stride
"""
import numpy as np

VSIZE = 0.025


def grid_axes(xyz):
    """prepare_zjumocap.py:152-165 -> the three float64 axes of the lattice over `xyz` (float64 in the tool)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    lo = np.min(xyz, axis=0)
    hi = np.max(xyz, axis=0)
    lo -= 0.05
    hi += 0.05
    return [np.arange(lo[a], hi[a] + VSIZE, VSIZE) for a in range(3)]


def lattice(xyz):
    """-> (origin (3) float64, step (3) float64, dims (3) int) of the header's lattice rule for the tool's axes, with the check that
    origin + i * step IS the tool's axis, bit for bit."""
    axes = grid_axes(xyz)
    origin = np.array([ax[0] for ax in axes])
    step = np.array([ax[1] - ax[0] for ax in axes])
    dims = [len(ax) for ax in axes]
    for a in range(3):
        assert np.array_equal(origin[a] + np.arange(dims[a]).astype(np.float64) * step[a], axes[a])
    return origin, step, dims


def lattice_points(origin, step, dims, index=None):
    """(n, 3) float64 lattice points of the header's rule, all of them in linear order (x slowest) or those at the linear `index`."""
    if index is None:
        index = np.arange(int(np.prod(dims)))
    ijk = np.stack(np.unravel_index(np.asarray(index), dims), axis=1)
    return np.asarray(origin, np.float64)[None] + ijk.astype(np.float64) * np.asarray(step, np.float64)[None]


def brute_force(verts, points, chunk=2048):
    """The contract: for each float64 point the lexicographic minimum of (d2, row) over the float32 `verts`, d2 =
    ((gx - vx)^2 + (gy - vy)^2) + (gz - vz)^2 in float64 in that order -> (dist float32 = float32(sqrt(d2)), nearest int32)."""
    v = np.asarray(verts, dtype=np.float32).astype(np.float64)
    points = np.asarray(points, dtype=np.float64)
    dist = np.empty(len(points), np.float32)
    near = np.empty(len(points), np.int32)
    for s in range(0, len(points), chunk):
        g = points[s:s + chunk]
        ex = g[:, None, 0] - v[None, :, 0]
        ey = g[:, None, 1] - v[None, :, 1]
        ez = g[:, None, 2] - v[None, :, 2]
        d2 = (ex * ex + ey * ey) + ez * ez
        r = np.argmin(d2, axis=1)                    # the first of equal minima: the lowest row
        near[s:s + chunk] = r
        dist[s:s + chunk] = np.sqrt(d2[np.arange(len(g)), r]).astype(np.float32)
    return dist, near


def get_bounds(xyz, padding=0.05):
    """if_nerf_data_utils.py:689-696."""
    lo = np.min(xyz, axis=0)
    hi = np.max(xyz, axis=0)
    lo -= padding
    hi += padding
    return np.stack([lo, hi], axis=0).astype(np.float32)


def pose_points(wxyz, Th, R):
    """tpose_dataset.py:270."""
    return np.dot(wxyz - Th, R).astype(np.float32)


def rigid_transformation(poses, joints, parents):
    """if_nerf_data_utils.py:523-577 (batch_rodrigues + get_rigid_transformation) in float64 -> A (24,4,4) float32."""
    poses = np.asarray(poses, np.float64).reshape(24, 3)
    joints = np.asarray(joints, np.float64)
    angle = np.linalg.norm(poses + 1e-8, axis=1, keepdims=True)
    d = poses / angle
    c, s = np.cos(angle)[:, None], np.sin(angle)[:, None]
    z = np.zeros(24)
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], axis=1).reshape(24, 3, 3)
    rot = np.eye(3)[None] + s * K + (1 - c) * np.matmul(K, K)
    rel = joints.copy()
    rel[1:] -= joints[parents[1:]]
    mats = np.zeros((24, 4, 4))
    mats[:, :3, :3] = rot
    mats[:, :3, 3] = rel
    mats[:, 3, 3] = 1
    chain = [mats[0]]
    for i in range(1, 24):
        chain.append(np.dot(chain[parents[i]], mats[i]))
    T = np.stack(chain, axis=0)
    jh = np.concatenate([joints, np.zeros((24, 1))], axis=1)
    T[..., 3] = T[..., 3] - np.sum(T * jh[:, None], axis=2)
    return T.astype(np.float32)


def exact_volume(verts, points, k=8):
    """The contract's (dist, nearest) on MANY points in seconds: a k-d tree proposes each point's k nearest rows and the contract's
    (d2, row) minimum is taken over them.  The tree's own distances are good to a few double ulps, so the contract's winner is among
    the k proposals unless k rows lie within a few ulps of each other at one point (the caller checks this on seeded points against
    brute_force)."""
    from scipy.spatial import cKDTree
    v = np.asarray(verts, np.float32).astype(np.float64)
    points = np.asarray(points, np.float64)
    k = min(k, len(v))
    _, rows = cKDTree(v).query(points, k=k)
    rows = np.sort(rows.reshape(len(points), k), axis=1)           # ascending rows: argmin's first minimum is the lowest row
    e = points[:, None, :] - v[rows]
    d2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    j = np.argmin(d2, axis=1)
    at = np.arange(len(points))
    return np.sqrt(d2[at, j]).astype(np.float32), rows[at, j].astype(np.int32)


def part_sets(ppts, weights, parts, tpose, n_parts, bbox_overlap):
    """tpose_dataset.py:570-600 -> part_pts, part_pbw, lengths2, bounds."""
    N, D = weights.shape
    part_pts = np.zeros((n_parts, N, 3), dtype=np.float32)
    part_pbw = np.zeros((n_parts, N, D), dtype=np.float32)
    lengths2 = np.zeros(n_parts, dtype=np.int64)
    bounds = np.zeros((n_parts, 2, 3), dtype=np.float32)
    for pid in range(n_parts):
        flag = parts == pid
        lengths2[pid] = np.count_nonzero(flag)
        part_pts[pid, :lengths2[pid]] = ppts[flag]
        part_pbw[pid, :lengths2[pid]] = weights[flag]
        bounds[pid, 0] = tpose[flag].min(axis=0) - bbox_overlap
        bounds[pid, 1] = tpose[flag].max(axis=0) + bbox_overlap
    m = lengths2.max()
    return part_pts[:, :m], part_pbw[:, :m], lengths2, bounds
