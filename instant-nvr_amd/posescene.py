"""Novel poses: a frame's scene tensors from SMPL output alone.

The reference prepares the pose-dependent tensors of a frame offline (tools/prepare_zjumocap.py: a 25-channel blend-weight volume per
frame, computed with psbody.mesh / CGAL) and its dataset loads them (lib/datasets/h36m/tpose_dataset.py:260-296, 570-600).  PoseScenes
builds them per frame from the posed vertices and the pose parameters: O(V) NumPy lines on the host, exactly the reference's, and on
the device the LBS matrices (invr_rigid_transformation), the per-part reference sets (invr_pack_parts) and the distance volume
(invr_distance_volume, include/invr_posescene.h).  The path reads only the last channel of `pbw` — the distance to the nearest vertex
(inb_part_network_multiassign.py:134) — so the volume built here has that one channel.

Novel subjects: the canonical volumes of a subject (`bigpose_uv.npy`, `bigpose_bw.npy`: get_bigpose_uv / get_bigpose_blend_weights of the
same tool, again psbody.mesh / CGAL) are built by canonical_volumes from the big-pose mesh and its per-vertex attributes through the
closest point on the surface (invr_surface_volume / invr_surface_interpolate, include/invr_surface.h); PoseScenes.from_smpl is the
constructor for a subject that has no precomputed volume."""
import numpy as np
import torch

from . import config as _config
from . import prep
from .config import NUM_PARTS

VSIZE = 0.025                  # tools/prepare_zjumocap.py:158
GRID_PADDING = 0.05            # tools/prepare_zjumocap.py:155-156


class PoseFrame(dict):
    """The un-batched scene dict of one posed frame (device tensors) — what TrainSet.add_frame(scene=...) and _abi.make_scene (with a
    leading batch dimension) understand — plus `host`: the values frame() computed on the host (wbounds, pbounds, origin, step, dims,
    latent_index, frame_index), so that nothing has to be read back."""
    host = None


def canonical_volumes(bigpose_vertices, faces, vertex_uv, weights=None, device='cuda', cfg=None):
    """A subject's canonical volumes from its big-pose SMPL mesh alone — what tools/prepare_zjumocap.py computes offline with
    psbody.mesh / CGAL: get_bigpose_uv (:177-240, `bigpose_uv.npy`) and, with `weights` (V,24), get_bigpose_blend_weights (:312-400,
    `bigpose_bw.npy`: the interpolated skinning weights and the distance to the surface as the last channel).  bigpose_vertices (V,3),
    faces (F,3), vertex_uv (V,2): host arrays.  The closest point of the surface for every lattice point and the interpolation are
    include/invr_surface.h's (the contract's brute force in double; not compared with CGAL's result, which is not available here).
    -> {'tuv' (Dx,Dy,Dz,2) float32 device tensor, 'tbounds' (2,3) float32 host array = get_bounds of the float32 vertices with
    cfg.box_padding, 'origin', 'step' (3) float64 and 'dims' of the lattice of get_grid_points over the float64 vertices
    [, 'tbw' (Dx,Dy,Dz,25)]}.  Asynchronous on the current stream."""
    cfg = _config.cfg if cfg is None else cfg
    device = torch.device(device)
    xyz = np.asarray(bigpose_vertices)
    if xyz.ndim != 2 or xyz.shape[1] != 3 or np.asarray(vertex_uv).shape != (xyz.shape[0], 2):
        raise ValueError('canonical_volumes: bigpose_vertices must be (V, 3) and vertex_uv (V, 2) (got %s, %s)' % (xyz.shape, np.asarray(vertex_uv).shape))
    if weights is not None and np.asarray(weights).shape != (xyz.shape[0], 24):
        raise ValueError('canonical_volumes: weights must be (V, 24) (got %s)' % (np.asarray(weights).shape,))
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).to(device)
    origin, step, dims = PoseScenes.lattice(xyz)
    x32 = np.ascontiguousarray(xyz, np.float32)
    lo, hi = np.min(x32, axis=0), np.max(x32, axis=0)          # get_bounds (if_nerf_data_utils.py:689-696)
    lo -= float(cfg.get('box_padding', 0.05))
    hi += float(cfg.get('box_padding', 0.05))
    d_faces = up(faces, np.int32)
    face, bary, dist = prep.surface_volume(up(x32, np.float32), d_faces, origin, step, dims)
    out = {'tuv': prep.surface_interpolate(up(vertex_uv, np.float32), d_faces, face, bary),
           'tbounds': np.stack([lo, hi], axis=0).astype(np.float32), 'origin': origin, 'step': step, 'dims': list(dims)}
    if weights is not None:
        tbw = torch.empty(list(dims) + [25], dtype=torch.float32, device=device)
        prep.surface_interpolate(up(weights, np.float32), d_faces, face, bary, out=tbw)
        tbw[..., 24] = dist
        out['tbw'] = tbw
    return out


class PoseScenes:
    @classmethod
    def from_smpl(cls, joints, parents, weights, parts, tpose, faces, vertex_uv, big_poses, cfg=None, device='cuda'):
        """A new subject: the constructor's arguments with the SMPL faces (F,3) and per-vertex UVs (V,2) in place of the precomputed
        canonical volume — `tuv` and `tbounds` are built by canonical_volumes from tpose (the big-pose vertices).  Once per subject: the
        volume takes the constructor's own way in, as a host array (one read-back)."""
        vol = canonical_volumes(tpose, faces, vertex_uv, device=device, cfg=cfg)
        return cls(joints, parents, weights, parts, tpose, vol['tuv'].cpu().numpy(), vol['tbounds'], big_poses, cfg=cfg, device=device)

    def __init__(self, joints, parents, weights, parts, tpose, tuv, tbounds, big_poses, cfg=None, device='cuda'):
        """The static data of a subject as the reference's dataset holds them (tpose_dataset.py: joints.npy (24,3), parents (24),
        meta_smpl's weights (V,24) and parts (V), bigpose_vertices.npy (V,3), the canonical bigpose_uv.npy volume and its bounds
        (2,3)), uploaded once.  big_poses (72) or (24,3): the canonical pose big_A is computed from — the reference has two
        definitions (tpose_dataset.py:278-288), so there is no default."""
        self.cfg = _config.cfg if cfg is None else cfg
        self.device = torch.device(device)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).to(self.device)
        self.joints, self.parents = up(joints, np.float64), up(parents, np.int32)
        self.weights, self.parts, self.tpose = up(weights, np.float32), up(parts, np.int64), up(tpose, np.float32)
        self.tuv, self.tbounds = up(tuv, np.float32), up(tbounds, np.float32)
        self.n_verts = self.weights.shape[0]
        if self.tpose.shape != (self.n_verts, 3) or self.parts.shape != (self.n_verts,):
            raise ValueError('PoseScenes: weights (V,24), parts (V) and tpose (V,3) disagree on V')
        self.big_A = prep.rigid_transformation(up(np.asarray(big_poses, np.float64).reshape(24, 3), np.float64), self.joints, self.parents)
        # static per subject: the per-part row counts and the trimmed stride of the part sets (tpose_dataset.py:591-593)
        self.lengths2 = np.bincount(np.asarray(parts, np.int64), minlength=NUM_PARTS)[:NUM_PARTS]
        self.max_length = int(self.lengths2.max())
        self.padding = float(self.cfg.get('box_padding', 0.05))
        self.bbox_overlap = float(self.cfg.get('bbox_overlap', 0.2))
        self.num_train_frame = float(self.cfg.get('num_train_frame', 100))
        self._side_stream = None

    # ---- host side: the reference's own lines ---------------------------------------------------------------------------------------
    def _bounds(self, xyz):
        """get_bounds (if_nerf_data_utils.py:689-696), float32 in, float32 out."""
        lo, hi = np.min(xyz, axis=0), np.max(xyz, axis=0)
        lo -= self.padding
        hi += self.padding
        return np.stack([lo, hi], axis=0).astype(np.float32)

    @staticmethod
    def lattice(ppts):
        """get_grid_points (tools/prepare_zjumocap.py:152-165) of the float64 vertices -> (origin, step, dims) of
        include/invr_posescene.h's lattice rule: origin + i * step reproduces np.arange's values."""
        xyz = ppts.astype(np.float64)
        lo, hi = np.min(xyz, axis=0), np.max(xyz, axis=0)
        lo -= GRID_PADDING
        hi += GRID_PADDING
        axes = [np.arange(lo[a], hi[a] + VSIZE, VSIZE) for a in range(3)]
        return np.array([ax[0] for ax in axes]), np.array([ax[1] - ax[0] for ax in axes]), [len(ax) for ax in axes]

    def _side(self):
        """The stream host-bound work runs on (None on a host device): a copy from pageable memory holds the host until it has run, and
        the ray count of a batch is read back — on the caller's stream either would wait for everything queued there."""
        if self.device.type != 'cuda':
            return None
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream(self.device)
        return self._side_stream

    def _join_side(self, tensors):
        """The caller's stream waits for the side stream's work; `tensors` (allocated there) are used on the caller's stream from now on."""
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self._side_stream)
        for t in tensors:
            t.record_stream(cur)

    def _to_device(self, arrays):
        """Host arrays -> device tensors, copied on the side stream."""
        side = self._side()
        if side is None:
            return [torch.from_numpy(a) for a in arrays]
        with torch.cuda.stream(side):
            out = [torch.from_numpy(a).to(self.device, non_blocking=True) for a in arrays]
        self._join_side(out)
        return out

    # ---- one frame ------------------------------------------------------------------------------------------------------------------
    def frame(self, wxyz, Th, poses, latent_index, R=None, Rh=None, frame_index=0):
        """wxyz (V,3) float32 world vertices, Th (3) translation, poses (72) axis-angle, and R (3,3) or Rh (3) — host arrays of one
        frame, as the reference reads them from vertices/{i}.npy and params/{i}.npy.  -> PoseFrame.  Nothing is read back and
        nothing synchronises: the device work is queued on the current stream."""
        if torch.is_tensor(wxyz):
            raise TypeError('PoseScenes.frame: wxyz must be a host array (the lattice is sized from its extent on the host)')
        wxyz = np.ascontiguousarray(wxyz, np.float32)
        if wxyz.shape != (self.n_verts, 3):
            raise ValueError('PoseScenes.frame: wxyz must be (%d, 3) (got %s)' % (self.n_verts, wxyz.shape))
        if R is None:
            if Rh is None:
                raise ValueError('PoseScenes.frame: give R (3,3) or Rh (3)')
            from .scene import rodrigues
            R = rodrigues(np.asarray(Rh, np.float64).reshape(3))
        R = np.asarray(R).astype(np.float32).reshape(3, 3)              # tpose_dataset.py:260
        Th = np.asarray(Th).astype(np.float32).reshape(1, 3)            # :259
        ppts = np.dot(wxyz - Th, R).astype(np.float32)                   # :270
        pbounds, wbounds = self._bounds(ppts), self._bounds(wxyz)
        origin, step, dims = self.lattice(ppts)
        frame_dim = np.float32(latent_index / self.num_train_frame)     # :497

        # the small tensors travel in one copy, each in a 256-byte slot of its own (the alignment separate allocations would have)
        small = np.zeros(5 * 64, np.float32)
        for slot, a in enumerate((pbounds, wbounds, R, Th, frame_dim)):
            small[64 * slot:64 * slot + a.size] = a.ravel()
        d_ppts, d_small, d_poses, d_latent = self._to_device([ppts, small, np.ascontiguousarray(np.asarray(poses, np.float64).reshape(24, 3)),
                                                              np.array(int(latent_index), np.int64)])
        A = prep.rigid_transformation(d_poses, self.joints, self.parents)
        part_pts, part_pbw, lengths2, bounds = prep.pack_parts(d_ppts, self.weights, self.parts, self.tpose, self.bbox_overlap,
                                                               max_length=self.max_length)
        dist = prep.distance_volume(d_ppts, origin, step, dims)
        f = PoseFrame(A=A, big_A=self.big_A, pbw=dist[..., None], pbounds=d_small[0:6].view(2, 3), wbounds=d_small[64:70].view(2, 3),
                      R=d_small[128:137].view(3, 3), Th=d_small[192:195].view(1, 3), ppts=d_ppts, part_pts=part_pts, part_pbw=part_pbw,
                      lengths2=lengths2, bounds=bounds, tuv=self.tuv, tbounds=self.tbounds, frame_dim=d_small[256], latent_index=d_latent)
        f.host = {'wbounds': wbounds, 'pbounds': pbounds, 'origin': origin, 'step': step, 'dims': dims, 'latent_index': int(latent_index),
                  'frame_index': int(frame_index)}
        return f

    def eval_batch(self, frame, H, W, K, R, T):
        """The collated full-frame eval batch (leading dimension 1) of a PoseFrame seen from the camera K (3,3), R (3,3), T (3,1):
        rays.rays_within_bounds on the frame's world box, mask_at_box, H, W and the scene tensors by reference — the shape of
        TrainSet.test_batch, for Renderer.render / driver.run_poses."""
        from . import rays
        side = self._side()
        if side is None:
            ray_o, ray_d, near, far, mask = rays.rays_within_bounds(int(H), int(W), K, R, T, frame.host['wbounds'], self.device)
        else:
            with torch.cuda.stream(side):             # (the ray count is read back: behind the ray kernel only, not behind the scene build)
                ray_o, ray_d, near, far, mask = rays.rays_within_bounds(int(H), int(W), K, R, T, frame.host['wbounds'], self.device)
            self._join_side((ray_o, ray_d, near, far, mask))
        batch = {'ray_o': ray_o[None], 'ray_d': ray_d[None], 'near': near[None], 'far': far[None], 'mask_at_box': mask.reshape(1, -1),
                 'H': torch.tensor([int(H)], dtype=torch.int64), 'W': torch.tensor([int(W)], dtype=torch.int64),
                 'frame_index': torch.tensor([frame.host['frame_index']], dtype=torch.int64)}
        batch.update({k: v[None] for k, v in frame.items()})
        return batch
