"""GPU: invr_perceptual_fwd + invr_perceptual_bwd captured in a hipGraph (one stream, no allocation, no read-back inside the calls) and
replayed on new input values give, bit for bit, what the plain calls give."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from invr import _abi                                # noqa: E402
from tests import test_gpu_perceptual as T           # noqa: E402

DEV = 'cuda:0'


def test_forward_and_backward_replay_in_a_graph():
    H, W, mask, rgb, gt = T.inputs('17x15-p80-0.05')
    L = _abi.lib()
    n = rgb.shape[0]
    nbytes = L.invr_perceptual_workspace_bytes(H, W)
    ws = T.aligned_bytes(nbytes, 0xFF)
    pk = T.packed()
    mask_d = mask.to(DEV)
    rgb_d, gt_d = torch.zeros(n, 3, device=DEV), torch.zeros(n, 3, device=DEV)
    out8, g_rgb = torch.zeros(8, device=DEV), torch.zeros(n, 3, device=DEV)
    gl = torch.tensor([T.G_LOSS], device=DEV)

    def calls():
        _abi.check(L.invr_perceptual_fwd(_abi.ptr(pk), _abi.ptr(rgb_d), _abi.ptr(gt_d), _abi.ptr(mask_d, torch.uint8), n, H, W,
                                         _abi.ptr(ws, torch.uint8), nbytes, _abi.ptr(out8), _abi.stream_ptr()))
        _abi.check(L.invr_perceptual_bwd(_abi.ptr(pk), _abi.ptr(mask_d, torch.uint8), n, H, W, _abi.ptr(ws, torch.uint8), nbytes, _abi.ptr(gl),
                                         _abi.ptr(g_rgb), _abi.stream_ptr()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        calls()
    rgb_d.copy_(rgb.to(DEV))                          # the values arrive after the capture
    gt_d.copy_(gt.to(DEV))
    for _ in range(2):
        ws.fill_(0x5A)
        out8.fill_(float('nan'))
        g_rgb.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        ref = T.run('17x15-p80-0.05', T.DEV)
        assert T.same_bits(out8.cpu(), ref['out8']) and T.same_bits(g_rgb.cpu(), ref['g_rgb'])
