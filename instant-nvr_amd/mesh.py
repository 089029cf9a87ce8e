"""A surface mesh of the posed human per frame (include/invr_mesh.h): the occupancy field on a regular grid over the frame's world
bounds, then marching tetrahedra on the device.  The reference's hooks for geometry — Trainer.tmesh (trainer.py:258-275),
run.py --type tmesh / tdmesh and the visualizer that turns output['occ'] into a .ply with cfg.voxel_size at level 0.1
(lib/visualizers/if_nerf.py:133-160) — lack their renderer and dataset in the released code and lean on CPU mcubes / trimesh; here
the grid, the field query (Network.forward = invr_field_fwd) and the extraction all stay on the device, and only the finished
mesh goes to the host, in write_ply."""
import ctypes as C

import numpy as np
import torch

from . import _abi

LEVEL = 0.1          # lib/visualizers/if_nerf.py:147 hard-codes it


def _c3(v, t):
    return (t * 3)(*[(float if t is C.c_float else int)(x) for x in v])


def _voxel(net, voxel_size):
    v = voxel_size if voxel_size is not None else net.cfg.get('voxel_size', [0.005, 0.005, 0.005])
    v = np.asarray(v, dtype=np.float32).reshape(-1)
    v = np.repeat(v, 3) if v.size == 1 else v
    if v.shape != (3,) or not (np.isfinite(v).all() and (v > 0).all()):
        raise ValueError('voxel_size must be one or three finite sizes > 0 (got %r)' % (voxel_size,))
    return v


def _aligned_bytes(nbytes, device):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)          # (the library asks for 256-byte alignment)
    off = (-raw.data_ptr()) % 256
    return raw[off:off + nbytes]


def grid_of(batch, voxel):
    """-> (origin (3,) fp32, dims (3,) int) of the grid over batch['wbounds']: origin = the low corner, dims = floor(extent / voxel) + 1."""
    wb = batch['wbounds'].detach().to('cpu', torch.float32).reshape(2, 3).numpy()
    dims = np.floor((wb[1].astype(np.float64) - wb[0].astype(np.float64)) / voxel.astype(np.float64)).astype(np.int64) + 1
    return wb[0].copy(), dims


def grid_points(origin, voxel, dims, first, n, device):
    """World coordinates (n, 3) of the grid points [first, first + n) in linear order (invr_grid_points)."""
    xyz = torch.empty(n, 3, device=device)
    _abi.check(_abi.lib().invr_grid_points(_c3(origin, C.c_float), _c3(voxel, C.c_float), _c3(dims, C.c_int32), first, n, _abi.ptr(xyz),
                                           _abi.stream_ptr()))
    return xyz


def occupancy_volume(net, batch, voxel_size=None, chunk=1 << 21):
    """-> (vol (Dx, Dy, Dz) fp32 on the device, origin (3,), voxel (3,)): the eval-mode occupancy of Network.forward on the grid over
    batch['wbounds'], filled chunk by chunk; the points are generated on the device.  The view direction is the constant (0, 0, 1):
    occupancy does not depend on it."""
    voxel = _voxel(net, voxel_size)
    origin, dims = grid_of(batch, voxel)
    total = int(dims.prod())
    if _abi.lib().invr_mesh_workspace_bytes(_c3(dims, C.c_int32)) == 0:
        raise ValueError('occupancy_volume: a grid of %d x %d x %d points is beyond the mesh path\'s limit of 2^27 padded points' % tuple(dims))
    device = batch['wbounds'].device
    chunk = max(1, min(int(chunk), total))
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            ctx = net.prepare(batch)
            vol = torch.empty(total, device=device)
            dirs = torch.zeros(chunk, 3, device=device)
            dirs[:, 2] = 1.0
            for first in range(0, total, chunk):
                n = min(chunk, total - first)
                out = net.forward(grid_points(origin, voxel, dims, first, n, device), dirs[:n], None, ctx)
                vol[first:first + n] = out['occ'].reshape(-1)
    finally:
        net.train(was_training)
    return vol.view(*[int(d) for d in dims]), origin, voxel


def marching_tetrahedra(vol, origin, voxel, level=LEVEL):
    """-> (vertices (V, 3) float32, triangles (F, 3) int32) on vol's device: the closed, outward-oriented level set of include/invr_mesh.h.
    count, one read-back of the two totals, allocation, emit."""
    L = _abi.lib()
    vol = vol.detach().to(torch.float32).contiguous()
    assert vol.dim() == 3, 'marching_tetrahedra: a (Dx, Dy, Dz) volume'
    dims = _c3(vol.shape, C.c_int32)
    nbytes = L.invr_mesh_workspace_bytes(dims)
    if nbytes == 0:
        raise ValueError('marching_tetrahedra: a volume of %d x %d x %d is empty or beyond 2^27 padded points' % tuple(vol.shape))
    ws = _aligned_bytes(nbytes, vol.device)
    counts = torch.empty(4, dtype=torch.int64, device=vol.device)
    _abi.check(L.invr_mesh_count(_abi.ptr(vol), dims, float(level), _abi.ptr(ws, torch.uint8), nbytes, _abi.ptr(counts, torch.int64), _abi.stream_ptr()))
    nv, nt = counts[:2].tolist()
    vertices = torch.empty(nv, 3, device=vol.device)
    triangles = torch.empty(nt, 3, dtype=torch.int32, device=vol.device)
    _abi.check(L.invr_mesh_emit(_abi.ptr(vol), dims, _c3(origin, C.c_float), _c3(voxel, C.c_float), float(level), _abi.ptr(ws, torch.uint8), nbytes,
                                _abi.ptr(vertices) if nv else None, nv, _abi.ptr(triangles, torch.int32) if nt else None, nt,
                                _abi.ptr(counts, torch.int64), _abi.stream_ptr()))
    if int(counts[2]):
        raise RuntimeError('marching_tetrahedra: the emit pass found more than the %d vertices / %d triangles the count pass reported' % (nv, nt))
    return vertices, triangles


def extract_mesh(net, batch, level=LEVEL, voxel_size=None, view_from=None):
    """The posed surface of one frame -> dict(vertices, triangles, dims, origin, voxel[, colors]) with the tensors on the device.
    view_from (3-vector, world): also colors (V, 3) = the field's rgb at the vertices seen from that point."""
    vol, origin, voxel = occupancy_volume(net, batch, voxel_size)
    vertices, triangles = marching_tetrahedra(vol, origin, voxel, level)
    out = {'vertices': vertices, 'triangles': triangles, 'dims': tuple(vol.shape), 'origin': origin, 'voxel': voxel}
    if view_from is not None:
        out['colors'] = vertex_colors(net, batch, vertices, view_from)
    return out


def vertex_colors(net, batch, vertices, view_from):
    """raw[:, :3] of Network.forward(vertices, normalize(vertices - view_from)), eval mode."""
    eye = torch.as_tensor(view_from, dtype=torch.float32, device=vertices.device).reshape(1, 3)
    if vertices.shape[0] == 0:
        return torch.empty(0, 3, device=vertices.device)
    dirs = torch.nn.functional.normalize(vertices - eye, dim=1)
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            return net.forward(vertices, dirs, None, batch)['raw'][0, :, :3].contiguous()
    finally:
        net.train(was_training)


def ply_header(n_vertices, n_triangles, colors):
    lines = ['ply', 'format binary_little_endian 1.0', 'element vertex %d' % n_vertices, 'property float x', 'property float y', 'property float z']
    if colors:
        lines += ['property uchar red', 'property uchar green', 'property uchar blue']
    lines += ['element face %d' % n_triangles, 'property list uchar int vertex_indices', 'end_header']
    return ('\n'.join(lines) + '\n').encode('ascii')


def write_ply(path, vertices, triangles, colors=None):
    """Binary little-endian PLY: float x y z (+ uchar red green blue, colors in [0, 1] rounded to 8 bits), faces as uchar 3 + three int."""
    v = vertices.detach().to('cpu', torch.float32).contiguous().numpy() if torch.is_tensor(vertices) else np.ascontiguousarray(vertices, dtype=np.float32)
    t = triangles.detach().to('cpu', torch.int32).contiguous().numpy() if torch.is_tensor(triangles) else np.ascontiguousarray(triangles, dtype=np.int32)
    assert v.ndim == 2 and v.shape[1] == 3 and t.ndim == 2 and t.shape[1] == 3
    if colors is not None:
        c = colors.detach().to('cpu', torch.float32).numpy() if torch.is_tensor(colors) else np.asarray(colors, dtype=np.float32)
        assert c.shape == v.shape
        vrec = np.empty(len(v), dtype=[('p', '<f4', 3), ('c', 'u1', 3)])
        vrec['c'] = np.clip(np.rint(np.nan_to_num(c) * 255.0), 0, 255).astype(np.uint8)
    else:
        vrec = np.empty(len(v), dtype=[('p', '<f4', 3)])
    vrec['p'] = v
    frec = np.empty(len(t), dtype=[('n', 'u1'), ('i', '<i4', 3)])
    frec['n'], frec['i'] = 3, t
    with open(path, 'wb') as f:
        f.write(ply_header(len(v), len(t), colors is not None))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())
    return path
