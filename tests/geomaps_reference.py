"""CHECKER ONLY — a float64 NumPy restatement of the three contracts of include/invr_geomaps.h, taking the fp32 inputs the kernels
take.  Nothing here is a product path."""
import numpy as np


def z_vals_f32(near, far, S, jitter=None):
    """The renderer's sample depths in its own fp32 arithmetic (csrc/pipeline.h sample_z; oracle/nvr_oracle.py states the same formula):
    t_i = i * step below the middle, 1 - (S - 1 - i) * step above, step = fp32(1 / (S - 1)); z = near (1 - t) + far t, every operation
    rounded to fp32; with jitter (R, S) in [0, 1): stratified between the mid-points of neighbouring samples."""
    f = np.float32
    near, far = np.asarray(near, f).reshape(-1, 1), np.asarray(far, f).reshape(-1, 1)
    step = f(1.0) / f(S - 1)
    i = np.arange(S)
    t = np.where(i < S // 2, step * i.astype(f), f(1.0) - step * (S - 1 - i).astype(f)).astype(f)[None]
    z = (near * (f(1.0) - t) + far * t).astype(f)
    if jitter is not None:
        mid = (f(0.5) * (z[:, 1:] + z[:, :-1])).astype(f)
        upper = np.concatenate([mid, z[:, -1:]], 1)
        lower = np.concatenate([z[:, :1], mid], 1)
        z = (lower + (upper - lower) * np.asarray(jitter, f)).astype(f)
    return z


def weights64(occ, eps):
    """render_weights in float64 from fp32 occupancies: w_i = occ_i * prod_{j<i} (1 - occ_j + eps)."""
    a = np.asarray(occ, np.float64)
    T = np.cumprod(1.0 - a + float(eps), axis=1)
    T = np.concatenate([np.ones_like(T[:, :1]), T[:, :-1]], 1)
    return a * T


def depth64(weights, z):
    """sum_i w_i z_i in float64 from fp32 weights and depths."""
    return (np.asarray(weights, np.float64) * np.asarray(z, np.float64)).sum(1)


def first_crossing(occ, z, level):
    """-> (surf_index int32 (R,), surf_depth float64 (R,), lo (R,), hi (R,)): the first sample with occ >= level in fp32 (a NaN is no
    crossing), the interpolated depth of the contract in float64 (a NaN in front of the crossing interpolates as 0) and the two sample
    depths it lies between (both z_0 for a crossing at sample 0, both 0 without one)."""
    occ = np.asarray(occ, np.float32)
    level = np.float32(level)
    R = occ.shape[0]
    with np.errstate(invalid='ignore'):
        cross = occ >= level
    idx = np.where(cross.any(1), cross.argmax(1), -1).astype(np.int32)
    z64, o64 = np.asarray(z, np.float64), np.nan_to_num(occ.astype(np.float64), nan=0.0)
    depth, lo, hi = np.zeros(R), np.zeros(R), np.zeros(R)
    for r in range(R):
        i = int(idx[r])
        if i == 0:
            depth[r] = lo[r] = hi[r] = z64[r, 0]
        elif i > 0:
            t = (float(level) - o64[r, i - 1]) / (o64[r, i] - o64[r, i - 1])
            depth[r] = z64[r, i - 1] + t * (z64[r, i] - z64[r, i - 1])
            lo[r], hi[r] = z64[r, i - 1], z64[r, i]
    return idx, depth, lo, hi


STENCIL = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def stencil64(ray_o, ray_d, surf_depth, rows, h):
    """-> (pts (6 n, 3) float64, x (n, 3) float64): x = o + surf_depth d of the listed rows, pts = x +- h e_k in the contract's order."""
    o, d = np.asarray(ray_o, np.float64)[rows], np.asarray(ray_d, np.float64)[rows]
    x = o + np.asarray(surf_depth, np.float64)[rows, None] * d
    pts = x[:, None, :] + float(np.float32(h)) * STENCIL[None]
    return pts.reshape(-1, 3), x


def normals64(occ6):
    """occ6 (n, 6) fp32 -> (normal (n, 3) float64, mask (n,) bool): -g / |g| of the central differences; zeros / False where |g|^2, formed
    in fp32 as (gx^2 + gy^2) + gz^2, is 0 or not finite."""
    o = np.asarray(occ6, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        g32 = np.stack([o[:, 0] - o[:, 1], o[:, 2] - o[:, 3], o[:, 4] - o[:, 5]], 1).astype(np.float32)
        n2 = ((g32[:, 0] * g32[:, 0] + g32[:, 1] * g32[:, 1]).astype(np.float32) + g32[:, 2] * g32[:, 2]).astype(np.float32)
        mask = np.isfinite(n2) & (n2 > 0)
        o64 = o.astype(np.float64)
        g = np.stack([o64[:, 0] - o64[:, 1], o64[:, 2] - o64[:, 3], o64[:, 4] - o64[:, 5]], 1)
        normal = np.zeros_like(g)
        normal[mask] = -g[mask] / np.sqrt((g[mask] ** 2).sum(1))[:, None]
    return normal, mask
