"""Per-pixel geometry of a posed frame (include/invr_geomaps.h): the expected depth, the first crossing of the occupancy level along
every ray and the surface normal there.  The reference's visualizer reads exactly these keys — output['depth_map']
(lib/visualizers/if_nerf.py:103-121), output['surf_normal'] and output['surf_mask'] (:63-81) — but its renderer never produced them
(inb_renderer.py:107 carries a commented-out depth_map).  Here the depth and the crossing come from the depth pass behind the
compositing (Network.render_rays(want_depth=True)), and the normal from the field's central differences at the surface point:
six occupancy queries (Network.forward = invr_field_fwd) per ray that hit.  Everything stays on the device."""
import torch

from . import _abi

LEVEL = 0.5          # the reference treats |tocc - 0.5| < 0.02 as the surface (inb_renderer.py:81)


def surface_stencil(ray_o, ray_d, surf_depth, rows, h):
    """-> (pts (6 n, 3), dirs (6 n, 3)): the points x +- h e_k around the surface point x = o + surf_depth d of every listed ray row
    (int32, ascending), in the order +x, -x, +y, -y, +z, -z, and the ray's direction repeated for each (invr_surface_stencil)."""
    n = rows.shape[0]
    pts = torch.empty(6 * n, 3, device=ray_o.device)
    dirs = torch.empty(6 * n, 3, device=ray_o.device)
    _abi.check(_abi.lib().invr_surface_stencil(_abi.ptr(ray_o), _abi.ptr(ray_d), _abi.ptr(surf_depth), _abi.ptr(rows, torch.int32), n, float(h),
                                               _abi.ptr(pts), _abi.ptr(dirs), _abi.stream_ptr()))
    return pts, dirs


def stencil_normals(occ6, rows, n_rays):
    """occ6 (n, 6): the occupancy at the stencil points of the listed rays -> (surf_normal (n_rays, 3), surf_mask (n_rays,) bool): the
    normalised negative central difference where it is defined, zeros and False elsewhere (invr_stencil_normals)."""
    normal = torch.zeros(n_rays, 3, device=occ6.device)
    mask = torch.zeros(n_rays, dtype=torch.uint8, device=occ6.device)
    _abi.check(_abi.lib().invr_stencil_normals(_abi.ptr(occ6), _abi.ptr(rows, torch.int32), rows.shape[0], _abi.ptr(normal),
                                               _abi.ptr(mask, torch.uint8), _abi.stream_ptr()))
    return normal, mask.bool()


def field_occupancy(net, ctx, pts, dirs, chunk=1 << 21):
    """occ (n,) of Network.forward at world points, chunk by chunk (as mesh.occupancy_volume fills its volume)."""
    n = pts.shape[0]
    occ = torch.empty(n, device=pts.device)
    for first in range(0, n, chunk):
        m = min(chunk, n - first)
        occ[first:first + m] = net.forward(pts[first:first + m], dirs[first:first + m], None, ctx)['occ'].reshape(-1)
    return occ


def geometry_maps(net, batch, level=None, h=0.005, normals=True, chunk=1 << 21):
    """The geometry maps of one frame over the rays of mask_at_box, as device tensors: depth_map (n,), surf_depth (n,), surf_mask (n,)
    bool, surf_normal (n, 3), acc_map (n,), rgb_map (n, 3).  level None: cfg.surface_level (0.5).  An eval-mode render without raw, then —
    normals=True — one read-back (the number of rays that cross the level, torch.nonzero), the six-point stencil of step h around every
    surface point, the field there and the central difference.  normals=False: surf_mask = the rays that cross, surf_normal zeros."""
    if level is None:
        level = float(net.cfg.get('surface_level', LEVEL))
    f = _abi.f32c
    ray_o, ray_d, near, far = f(batch['ray_o'][0]), f(batch['ray_d'][0]), f(batch['near'][0]), f(batch['far'][0])
    n = ray_o.shape[0]
    was_training = net.training
    net.eval()
    try:
        with torch.no_grad():
            ctx = net.prepare(batch)
            out = net.render_rays(ctx, ray_o, ray_d, near, far, int(net.cfg.N_samples), want_raw=False, want_depth=True, level=level)
            hit = out['surf_index'] >= 0
            maps = {'depth_map': out['depth_map'], 'surf_depth': out['surf_depth'], 'acc_map': out['acc_map'], 'rgb_map': out['rgb_map']}
            if normals:
                rows = torch.nonzero(hit).reshape(-1).to(torch.int32)          # (ascending; the one read-back: its length)
                if rows.shape[0]:
                    pts, dirs = surface_stencil(ray_o, ray_d, out['surf_depth'], rows, h)
                    occ6 = field_occupancy(net, ctx, pts, dirs, chunk).view(-1, 6)
                    maps['surf_normal'], maps['surf_mask'] = stencil_normals(occ6, rows, n)
                else:
                    maps['surf_normal'], maps['surf_mask'] = torch.zeros(n, 3, device=ray_o.device), hit
            else:
                maps['surf_normal'], maps['surf_mask'] = torch.zeros(n, 3, device=ray_o.device), hit
    finally:
        net.train(was_training)
    return maps


def image_of(values, batch):
    """A per-ray map (n,) or (n, C) over the rays of mask_at_box -> (H, W) or (H, W, C) on the same device, zeros (False) elsewhere."""
    H, W = int(batch['H'].reshape(-1)[0]), int(batch['W'].reshape(-1)[0])
    mask = batch['mask_at_box'][0].reshape(-1).to(values.device).bool()
    img = torch.zeros((H * W,) + tuple(values.shape[1:]), dtype=values.dtype, device=values.device)
    img[mask] = values
    return img.view((H, W) + tuple(values.shape[1:]))
