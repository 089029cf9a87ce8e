"""GPU: invr_lpips_fwd (keep = 0, the production mode) captured in a hipGraph (one stream, no allocation, no read-back inside the call)
and replayed on new input values gives, bit for bit, what the plain call gives."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from invr import _abi                                # noqa: E402
from tests import test_gpu_lpips as T                # noqa: E402

DEV = 'cuda:0'
CASE = '37x53-rand-0.05'


def test_forward_replays_in_a_graph():
    pred, gt = T.inputs(CASE)
    H, W = pred.shape[:2]
    L = _abi.lib()
    nbytes = L.invr_lpips_workspace_bytes(H, W, 0)
    ws = T.aligned_bytes(nbytes, 0xFF)
    pk = T.packed()
    pred_d, gt_d = torch.zeros(H, W, 3, device=DEV), torch.zeros(H, W, 3, device=DEV)
    out8 = torch.zeros(8, dtype=torch.float64, device=DEV)

    def call():
        _abi.check(L.invr_lpips_fwd(_abi.ptr(pk), _abi.ptr(pred_d), _abi.ptr(gt_d), H, W, 0, _abi.ptr(ws, torch.uint8), C.c_size_t(nbytes),
                                    _abi.ptr(out8, torch.float64), _abi.stream_ptr()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        call()
    pred_d.copy_(pred.to(DEV))                        # the values arrive after the capture
    gt_d.copy_(gt.to(DEV))
    ref = T.run(CASE, T.DEV)
    for _ in range(2):
        ws.fill_(0x5A)
        out8.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert T.same_bits(out8.cpu(), ref['out8'])
