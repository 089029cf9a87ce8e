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
