"""GPU: the mesh path's Python layers (invr.mesh, driver.run_mesh) on the golden scene at a 0.04 m grid: the occupancy volume is,
bit for bit, Network.forward (pinned to the reference by tests/test_gpu_parity.py) on the explicitly built point list, with chunks
smaller than the grid and a ragged last one; the extracted surface is closed, oriented and inside the frame's bounds; the vertex
colours are a direct field query; the .ply file round-trips byte for byte."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mesh_reference as R                # noqa: E402  (checker only)
from invr import driver, mesh                        # noqa: E402
from invr.network import Network                     # noqa: E402

DEV = 'cuda:0'
VOXEL = 0.04
EYE = (0.3, -2.5, 0.9)


@pytest.fixture(scope='module')
def setup(small_setup):
    cfg, sd, batch, _ = small_setup
    net = Network(cfg=cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    gb = {k: v.to(DEV) for k, v in batch.items()}
    return net, gb


@pytest.fixture(scope='module')
def extracted(setup):
    net, gb = setup
    return mesh.extract_mesh(net, gb, level=0.1, voxel_size=VOXEL, view_from=EYE)


def same_bits(a, b):
    return a.shape == b.shape and bool((a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)).all())


def test_occupancy_volume_is_network_forward_on_the_grid(setup):
    net, gb = setup
    vol, origin, voxel = mesh.occupancy_volume(net, gb, voxel_size=VOXEL, chunk=1000)
    wb = gb['wbounds'].reshape(2, 3).cpu().numpy()
    dims = tuple(vol.shape)
    assert np.array_equal(origin, wb[0]) and np.array_equal(voxel, np.full(3, VOXEL, dtype=np.float32))
    assert dims == tuple(int(np.floor((float(wb[1][a]) - float(wb[0][a])) / float(np.float32(VOXEL))) + 1) for a in range(3))
    total = int(np.prod(dims))
    assert 2000 < total < 100000 and total % 1000 != 0         # several chunks and a ragged last one
    idx = np.stack(np.unravel_index(np.arange(total), dims), axis=1)
    pts = torch.from_numpy(R.coords(origin, voxel, idx + 1)).to(DEV)          # (the checker's indices are padded ones)
    dirs = torch.zeros(total, 3, device=DEV)
    dirs[:, 2] = 1.0
    with torch.no_grad():
        want = net.forward(pts, dirs, None, gb)['occ'].reshape(dims)
    assert same_bits(vol, want)
    assert int((vol != 0).sum()) > 100 and float(vol.max()) > 0.1
    whole, _, _ = mesh.occupancy_volume(net, gb, voxel_size=VOXEL)          # one chunk
    assert same_bits(whole, vol)
    assert not net.training


def test_extract_mesh_is_closed_oriented_and_inside_the_bounds(setup, extracted):
    net, gb = setup
    m = extracted
    v, t = m['vertices'].cpu().numpy().astype(np.float64), m['triangles'].cpu().numpy()
    assert m['vertices'].dtype == torch.float32 and m['triangles'].dtype == torch.int32 and m['vertices'].is_cuda
    assert len(v) > 100 and len(t) > 200
    closed, chi = R.mesh_facts(len(v), t)
    assert closed and chi % 2 == 0
    assert (np.cross(v[t[:, 0]], v[t[:, 1]]) * v[t[:, 2]]).sum() > 0          # faces outward
    wb = gb['wbounds'].reshape(2, 3).cpu().numpy().astype(np.float64)
    assert (v >= wb[0] - VOXEL).all() and (v <= wb[1] + VOXEL).all()
    # the same volume through the C-ABI test's checker: counts and positions
    vol, origin, voxel = mesh.occupancy_volume(net, gb, voxel_size=VOXEL)
    ref = R.Reference(vol.cpu().numpy(), origin, voxel, 0.1)
    assert (len(v), len(t)) == (ref.n_vertices, ref.n_triangles)
    assert (np.abs(v - ref.positions) <= 8 * 2.0 ** -24 * (np.abs(ref.pa) + np.abs(ref.pb))).all()


def test_vertex_colours_are_a_direct_field_query(setup, extracted):
    net, gb = setup
    m = extracted
    c = m['colors']
    assert c.shape == m['vertices'].shape and float(c.min()) >= 0.0 and float(c.max()) <= 1.0
    eye = torch.tensor(EYE, device=DEV)
    dirs = torch.nn.functional.normalize(m['vertices'] - eye[None], dim=1)
    with torch.no_grad():
        want = net.forward(m['vertices'], dirs, None, gb)['raw'][0, :, :3]
    assert same_bits(c, want)
    assert 'colors' not in mesh.extract_mesh(net, gb, voxel_size=0.08)          # (and the level's default is the visualizer's 0.1)


def read_ply(path):
    """A reader for exactly the files write_ply writes -> (header bytes, vertex bytes, face bytes, properties)."""
    blob = open(path, 'rb').read()
    end = blob.index(b'end_header\n') + len(b'end_header\n')
    lines = blob[:end].decode('ascii').split('\n')
    nv = int([l for l in lines if l.startswith('element vertex')][0].split()[2])
    nf = int([l for l in lines if l.startswith('element face')][0].split()[2])
    props = [l for l in lines if l.startswith('property')]
    vsize = 12 + sum('uchar' in p and 'list' not in p for p in props)
    assert len(blob) == end + nv * vsize + nf * 13
    return blob[:end], blob[end:end + nv * vsize], blob[end + nv * vsize:], props


@pytest.mark.parametrize('colored', [False, True])
def test_write_ply_round_trips(extracted, tmp_path, colored):
    m = extracted
    v, t = m['vertices'].cpu().numpy(), m['triangles'].cpu().numpy()
    c = m['colors'].cpu().numpy() if colored else None
    path = mesh.write_ply(str(tmp_path / 'm.ply'), m['vertices'], m['triangles'], m['colors'] if colored else None)
    header, vbytes, fbytes, props = read_ply(path)
    want = 'ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n' % len(v)
    if colored:
        want += 'property uchar red\nproperty uchar green\nproperty uchar blue\n'
    want += 'element face %d\nproperty list uchar int vertex_indices\nend_header\n' % len(t)
    assert header == want.encode('ascii')
    if colored:
        rec = np.frombuffer(vbytes, dtype=[('p', '<f4', 3), ('c', 'u1', 3)])
        assert np.array_equal(rec['p'].view(np.int32), v.view(np.int32))
        assert np.array_equal(rec['c'], np.rint(c.astype(np.float32) * 255.0).astype(np.uint8))
    else:
        assert vbytes == v.astype('<f4').tobytes()
    faces = np.frombuffer(fbytes, dtype=[('n', 'u1'), ('i', '<i4', 3)])
    assert (faces['n'] == 3).all() and np.array_equal(faces['i'], t)


def test_run_mesh_writes_one_file_per_batch(setup, extracted, tmp_path, small_setup):
    net, _ = setup
    batch = small_setup[2]                            # host tensors: run_mesh moves them
    out = driver.run_mesh(net, [batch, batch], str(tmp_path), voxel_size=VOXEL, view_from=EYE, device=DEV)
    nv, nt = extracted['vertices'].shape[0], extracted['triangles'].shape[0]
    assert out['vertices'] == [nv, nv] and out['triangles'] == [nt, nt] and len(out['paths']) == 2
    assert len(set(out['paths'])) == 2 and all(os.path.exists(p) for p in out['paths'])
    header, vbytes, fbytes, _ = read_ply(out['paths'][1])
    assert len(vbytes) == nv * 15 and len(fbytes) == nt * 13
