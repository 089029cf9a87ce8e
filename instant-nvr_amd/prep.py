"""Row f4 of SURVEY.md §8: per-frame scene tensors on the device (no CPU dataset in the loop)."""
import ctypes as C

import torch

from . import _abi
from .config import NUM_PARTS


def rigid_transformation(poses, joints, parents):
    """get_rigid_transformation (if_nerf_data_utils.py:545-577): poses, joints (24,3), parents (24) -> A (24,4,4) f32."""
    dev = poses.device
    p = poses.to(torch.float64).contiguous()
    j = joints.to(torch.float64).contiguous()
    par = parents.to(torch.int32).contiguous()
    A = torch.empty(24, 4, 4, device=dev)
    _abi.check(_abi.lib().invr_rigid_transformation(_abi.ptr(p, torch.float64), _abi.ptr(j, torch.float64),
                                                    _abi.ptr(par, torch.int32), _abi.ptr(A), _abi.stream_ptr()))
    return A


def pack_parts(ppts, weights, parts, tpose, bbox_overlap=0.2, max_length=None):
    """tpose_dataset.py:570-600 -> part_pts (5,M,3), part_pbw (5,M,24), lengths2 (5) int64, bounds (5,2,3).
    max_length: M = max(lengths2) when the caller knows it (`parts` is static per subject): no read-back, no synchronisation."""
    dev = ppts.device
    V, W = weights.shape
    f = lambda t: t.to(torch.float32).contiguous()
    part_pts = torch.empty(NUM_PARTS, V, 3, device=dev)
    part_pbw = torch.empty(NUM_PARTS, V, W, device=dev)
    lengths2 = torch.empty(NUM_PARTS, dtype=torch.int64, device=dev)
    bounds = torch.empty(NUM_PARTS, 2, 3, device=dev)
    ppts, weights, tpose, parts = f(ppts), f(weights), f(tpose), parts.to(torch.int64).contiguous()      # held: pointers outlive the call
    _abi.check(_abi.lib().invr_pack_parts(_abi.ptr(ppts), _abi.ptr(weights), _abi.ptr(parts, torch.int64),
                                          _abi.ptr(tpose), V, W, V, float(bbox_overlap), _abi.ptr(part_pts), _abi.ptr(part_pbw),
                                          _abi.ptr(lengths2, torch.int64), _abi.ptr(bounds), _abi.stream_ptr()))
    M = int(lengths2.max()) if max_length is None else int(max_length)      # max_length trim (:591-593); unknown: one host sync as in NumPy
    return part_pts[:, :M].contiguous(), part_pbw[:, :M].contiguous(), lengths2, bounds


_DV_WORKSPACES = {}          # (device, stream) -> 256-byte aligned uint8 view: calls on one stream are ordered, so they share one


def _dv_workspace(nbytes, dev):
    key = (str(dev), _abi.stream_ptr().value)
    ws = _DV_WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        off = (-raw.data_ptr()) % 256
        ws = _DV_WORKSPACES[key] = raw[off:off + nbytes]
    return ws


def distance_volume(ppts, origin, step, dims, nearest=False):
    """include/invr_posescene.h: ppts (V,3) float32 device vertices; origin, step (3) float64 and dims (3) host values of the lattice
    g_a(i) = origin[a] + i * step[a] -> dist (Dx,Dy,Dz) float32, the distance from every lattice point to its nearest vertex, and with
    nearest=True also that vertex's row (Dx,Dy,Dz) int32 (ties: the lowest row).  Asynchronous on the current stream."""
    dev = ppts.device
    v = _abi.f32c(ppts)
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError('distance_volume: ppts must be (V, 3) (got %s)' % (tuple(ppts.shape),))
    dims = [int(d) for d in dims]
    L = _abi.lib()
    n = v.shape[0]
    nbytes = L.invr_distance_volume_workspace_bytes(n)
    if nbytes == 0:
        raise ValueError('distance_volume: the number of vertices must be in [1, 2^20] (got %d)' % n)
    if min(dims) < 1:
        raise ValueError('distance_volume: every dimension must be >= 1 (got %s)' % (dims,))
    ws = _dv_workspace(nbytes, dev)
    dist = torch.empty(dims, dtype=torch.float32, device=dev)
    near = torch.empty(dims, dtype=torch.int32, device=dev) if nearest else None
    _abi.check(L.invr_distance_volume(_abi.ptr(v), n, (C.c_double * 3)(*[float(x) for x in origin]), (C.c_double * 3)(*[float(x) for x in step]),
                                      (C.c_int32 * 3)(*dims), _abi.ptr(dist), _abi.ptr(near, torch.int32), _abi.ptr(ws, torch.uint8), ws.numel(),
                                      _abi.stream_ptr()))
    return (dist, near) if nearest else dist


def _lattice_args(who, origin, step, dims):
    dims = [int(d) for d in dims]
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError('%s: dims must be three dimensions >= 1 (got %s)' % (who, dims))
    return (C.c_double * 3)(*[float(x) for x in origin]), (C.c_double * 3)(*[float(x) for x in step]), (C.c_int32 * 3)(*dims), dims


def surface_volume(verts, faces, origin, step, dims, bary=True, dist=True):
    """include/invr_surface.h: verts (V,3) float32 and faces (F,3) int32 device tensors; origin, step (3) float64 and dims (3) host values
    of the lattice g_a(i) = origin[a] + i * step[a] -> face (Dx,Dy,Dz) int32, the face holding the closest point of the mesh for every
    lattice point (-1: no face takes part), with bary=True its barycentric coordinates (Dx,Dy,Dz,3) float64, with dist=True the
    distance (Dx,Dy,Dz) float32: (face[, bary][, dist]).  Asynchronous on the current stream; the workspace is cached per stream as
    distance_volume caches its own (and shared with it: calls on one stream are ordered)."""
    dev = verts.device
    v = _abi.f32c(verts)
    f = faces.to(torch.int32).contiguous()
    if v.dim() != 2 or v.shape[1] != 3 or f.dim() != 2 or f.shape[1] != 3:
        raise ValueError('surface_volume: verts must be (V, 3) and faces (F, 3) (got %s, %s)' % (tuple(verts.shape), tuple(faces.shape)))
    L = _abi.lib()
    nbytes = L.invr_surface_volume_workspace_bytes(f.shape[0])
    if nbytes == 0 or not 1 <= v.shape[0] <= 1 << 20:
        raise ValueError('surface_volume: the numbers of vertices and faces must be in [1, 2^20] (got %d, %d)' % (v.shape[0], f.shape[0]))
    o, s, d, dims = _lattice_args('surface_volume', origin, step, dims)
    ws = _dv_workspace(nbytes, dev)
    face = torch.empty(dims, dtype=torch.int32, device=dev)
    b = torch.empty(dims + [3], dtype=torch.float64, device=dev) if bary else None
    ds = torch.empty(dims, dtype=torch.float32, device=dev) if dist else None
    _abi.check(L.invr_surface_volume(_abi.ptr(v), v.shape[0], _abi.ptr(f, torch.int32), f.shape[0], o, s, d, _abi.ptr(face, torch.int32),
                                     _abi.ptr(b, torch.float64), _abi.ptr(ds), _abi.ptr(ws, torch.uint8), ws.numel(), _abi.stream_ptr()))
    return (face,) + ((b,) if bary else ()) + ((ds,) if dist else ())


def surface_interpolate(attr, faces, face, bary, out=None, offset=0):
    """include/invr_surface.h: attr (V,C) float32 per-vertex attributes, faces (F,3) int32, face (...) int32 and bary (...,3) float64 as
    surface_volume returns them -> (..., C) float32, (u A0 + v A1) + w A2 in double per channel, 0 where face = -1.  With `out`
    (..., C') float32 contiguous, C' >= offset + C: written into out[..., offset:offset + C] (the other channels are left alone) and
    returned."""
    dev = attr.device
    a = _abi.f32c(attr)
    f = faces.to(torch.int32).contiguous()
    fc = face.to(torch.int32).contiguous()
    b = bary.to(torch.float64).contiguous()
    if a.dim() != 2 or f.dim() != 2 or f.shape[1] != 3 or tuple(b.shape) != tuple(fc.shape) + (3,):
        raise ValueError('surface_interpolate: attr must be (V, C), faces (F, 3), bary face.shape + (3,) (got %s, %s, %s, %s)'
                         % (tuple(attr.shape), tuple(faces.shape), tuple(face.shape), tuple(bary.shape)))
    nc, offset = a.shape[1], int(offset)
    if not 1 <= nc <= 64 or not 1 <= a.shape[0] <= 1 << 20 or not 1 <= f.shape[0] <= 1 << 20:
        raise ValueError('surface_interpolate: need 1 <= C <= 64 and V, F in [1, 2^20] (got C %d, V %d, F %d)' % (nc, a.shape[0], f.shape[0]))
    if out is None:
        if offset != 0:
            raise ValueError('surface_interpolate: an offset needs `out`')
        out = torch.empty(tuple(fc.shape) + (nc,), dtype=torch.float32, device=dev)
    elif (out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device or tuple(out.shape[:-1]) != tuple(fc.shape) or offset < 0
          or offset + nc > out.shape[-1]):
        raise ValueError('surface_interpolate: out must be a contiguous float32 %s + (C\',) with offset + %d <= C\' (got %s, offset %d)'
                         % (tuple(fc.shape), nc, tuple(out.shape), offset))
    _abi.check(_abi.lib().invr_surface_interpolate(_abi.ptr(a), a.shape[0], nc, _abi.ptr(f, torch.int32), f.shape[0], _abi.ptr(fc, torch.int32),
                                                   _abi.ptr(b, torch.float64), fc.numel(), _abi.ptr(out), out.shape[-1], offset, _abi.stream_ptr()))
    return out
