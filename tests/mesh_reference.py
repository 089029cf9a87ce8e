"""CHECKER ONLY — a NumPy / float64 restatement of the marching-tetrahedra contract of include/invr_mesh.h, written from the contract's
text and sharing nothing with csrc/k_mesh.hip: the padded grid, the inside test, the per-point masks of crossed owned edges, the
vertex list in the contract's order with exact (float64) positions from the same fp32 inputs, the per-tetrahedron triangle counts
and the gradient of each tetrahedron's linear interpolant.  The triangle list itself is not restated: the tests hold it to the
properties the contract gives it (each triangle on one tetrahedron of its cell, closed, consistently oriented against the gradient)."""
import itertools

import numpy as np

SLOT_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
AXIS_ORDERS = tuple(itertools.permutations(range(3)))          # xyz, xzy, yxz, yzx, zxy, zyx


def tet_corners(order):
    """The four corners (offsets in {0,1}^3) of the path 000 -> +e_a -> +e_a+e_b -> 111."""
    c = [np.zeros(3, dtype=np.int64)]
    for a in order:
        nxt = c[-1].copy()
        nxt[a] = 1
        c.append(nxt)
    return np.stack(c)


TETS = np.stack([tet_corners(o) for o in AXIS_ORDERS])           # (6, 4, 3)


def padded(vol):
    """fp32 (Dx+2, Dy+2, Dz+2): the volume inside a border of zeros; a NaN reads as 0."""
    vol = np.asarray(vol, dtype=np.float32)
    p = np.zeros(tuple(d + 2 for d in vol.shape), dtype=np.float32)
    p[1:-1, 1:-1, 1:-1] = np.where(np.isnan(vol), np.float32(0), vol)
    return p


def coords(origin, voxel, idx):
    """fp32 positions of padded indices idx (n, 3): origin + (idx - 1) * voxel, product and sum rounded separately."""
    o, v = np.asarray(origin, dtype=np.float32), np.asarray(voxel, dtype=np.float32)
    prod = ((idx - 1).astype(np.float32) * v[None, :]).astype(np.float32)
    return (o[None, :] + prod).astype(np.float32)


def shifted(a, d, fill):
    """a[i + d] with `fill` beyond the grid."""
    out = np.full(a.shape, fill, dtype=a.dtype)
    sx, sy, sz = a.shape
    out[:sx - d[0], :sy - d[1], :sz - d[2]] = a[d[0]:, d[1]:, d[2]:]
    return out


class Reference:
    def __init__(self, vol, origin, voxel, level):
        level = np.float32(level)
        self.P = padded(vol)
        self.shape = self.P.shape
        self.inside = self.P >= level
        I = self.inside
        crossed = np.stack([I != shifted(I, d, False) for d in SLOT_DIRS], axis=-1)          # (Px, Py, Pz, 7); beyond the grid = outside = the border
        self.masks = ((crossed * (1 << np.arange(7))).sum(-1) + 128 * I).astype(np.uint8).reshape(-1)
        # vertices: by linear index of the owning point, then by slot (row-major nonzero of the (NP, 7) matrix)
        g, slot = np.nonzero(crossed.reshape(-1, 7))
        self.vert_point, self.vert_slot = g, slot
        ia = np.stack(np.unravel_index(g, self.shape), axis=1)
        ib = ia + np.asarray(SLOT_DIRS)[slot]
        self.vert_a, self.vert_b = ia, ib
        self.pa, self.pb = coords(origin, voxel, ia), coords(origin, voxel, ib)
        va, vb = self.P[tuple(ia.T)].astype(np.float64), self.P[tuple(ib.T)].astype(np.float64)
        t = (np.float64(level) - va) / (vb - va)
        self.t = t
        self.positions = self.pa.astype(np.float64) + t[:, None] * (self.pb.astype(np.float64) - self.pa.astype(np.float64))
        self.voffsets = np.concatenate([[0], np.cumsum(crossed.reshape(-1, 7).sum(1))[:-1]]).astype(np.int64)
        # per-tetrahedron triangle counts of every cell (0 where a point carries no cell) and corner values
        tet_in = np.stack([np.stack([shifted(I, c, False) for c in tet], -1) for tet in TETS], -2)          # (.., 6, 4)
        n_in = tet_in.sum(-1)
        self.tet_counts = np.where(n_in % 2 == 1, 1, np.where(n_in == 2, 2, 0)).reshape(-1, 6)
        self.tcounts = self.tet_counts.sum(1)
        self.toffsets = np.concatenate([[0], np.cumsum(self.tcounts)[:-1]]).astype(np.int64)
        self.n_vertices, self.n_triangles = len(g), int(self.tcounts.sum())
        self.voxel = np.asarray(voxel, dtype=np.float32).astype(np.float64)

    def gradient(self, cell, tet):
        """World-space gradient (n, 3) of the linear interpolant of tetrahedron `tet` (n,) of cell `cell` (n,): along the path
        000 -> +e_a -> +e_a+e_b -> 111 the value changes by v1 - v0 over voxel_a, v2 - v1 over voxel_b, v3 - v2 over voxel_c."""
        base = np.stack(np.unravel_index(cell, self.shape), axis=1)
        grad = np.zeros((len(cell), 3))
        vals = [self.P[tuple((base + TETS[tet][:, q]).T)].astype(np.float64) for q in range(4)]
        order = np.asarray(AXIS_ORDERS)[tet]
        for q in range(3):
            ax = order[:, q]
            grad[np.arange(len(cell)), ax] = (vals[q + 1] - vals[q]) / self.voxel[ax]
        return grad

    def triangle_tets(self, triangles, cells):
        """For triangles (F, 3) of vertex indices lying in cells (F,): the tetrahedron 0..5 of the cell whose four corners are exactly
        the ends of the three crossed edges, or -1 where there is none."""
        base = np.stack(np.unravel_index(cells, self.shape), axis=1)
        ends = np.concatenate([self.vert_a[triangles], self.vert_b[triangles]], axis=1) - base[:, None, :]          # (F, 6, 3)
        ok = ((ends >= 0) & (ends <= 1)).all(axis=(1, 2))
        code = np.where(ok[:, None], (np.clip(ends, 0, 1) * np.array([4, 2, 1])).sum(-1), 0)
        have = np.zeros((len(triangles), 8), dtype=bool)
        have[np.arange(len(triangles))[:, None], code] = True
        tet = np.full(len(triangles), -1)
        for t in range(6):
            want = np.zeros(8, dtype=bool)
            want[(TETS[t] * np.array([4, 2, 1])).sum(-1)] = True
            tet[ok & (have == want[None]).all(1)] = t
        return tet


def mesh_facts(n_vertices, triangles):
    """-> (closed_and_oriented, euler): every directed edge of the triangle list occurs exactly once and so does its reverse."""
    tri = np.asarray(triangles, dtype=np.int64)
    if len(tri) == 0:
        return n_vertices == 0, 0
    e = np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]])
    if (e[:, 0] == e[:, 1]).any():
        return False, None
    key, rev = e[:, 0] * (n_vertices + 1) + e[:, 1], e[:, 1] * (n_vertices + 1) + e[:, 0]
    uniq = len(np.unique(key)) == len(key)
    closed = uniq and bool(np.isin(rev, key).all())
    used = len(np.unique(tri)) == n_vertices
    return closed and used, n_vertices - len(key) // 2 + len(tri)
