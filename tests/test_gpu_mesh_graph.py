"""GPU: invr_mesh_count + invr_mesh_emit captured in a hipGraph (one stream, no allocation, no read-back inside the calls) and replayed
on a volume that arrives after the capture give, bit for bit, what the plain calls give."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from invr import _abi                                # noqa: E402
from tests import test_gpu_mesh as T                 # noqa: E402

DEV = 'cuda:0'


def test_count_and_emit_replay_in_a_graph():
    case = '17x9x33'
    vol = T.volume(case)
    ref = T.run(case, T.DEV)
    nv, nt = ref['n_vertices'], ref['n_triangles']
    L = _abi.lib()
    ws = T.aligned_bytes(L.invr_mesh_workspace_bytes(T.c3(vol.shape, C.c_int32)), 0xFF)
    vol_d = torch.zeros(vol.shape, device=DEV)
    counts = torch.zeros(4, dtype=torch.int64, device=DEV)
    verts, tris = torch.zeros(nv, 3, device=DEV), torch.zeros(nt, 3, dtype=torch.int32, device=DEV)

    def calls():
        T.count(vol_d, vol.shape, T.LEVEL, ws, counts)
        T.emit(vol_d, vol.shape, T.ORIGIN, T.VOXEL, T.LEVEL, ws, verts, nv, tris, nt, counts)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        calls()
    vol_d.copy_(torch.from_numpy(vol))               # the values arrive after the capture
    for _ in range(2):
        ws.fill_(0x5A)
        verts.fill_(float('nan'))
        tris.fill_(-1)
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        assert counts.tolist() == [nv, nt, 0, 0]
        assert T.same_bits(verts.cpu(), ref['vertices']) and torch.equal(tris.cpu(), ref['triangles'])
