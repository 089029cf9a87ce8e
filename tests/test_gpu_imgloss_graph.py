"""GPU: the SSIM and TV terms' forward + backward captured in a hipGraph (one stream, no allocation, no read-back inside the calls) and
replayed on new input values give, bit for bit, what the plain calls give."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from invr import _abi                                # noqa: E402
from tests import imgloss_reference as R             # noqa: E402
from tests import test_gpu_imgloss as T              # noqa: E402

DEV = 'cuda:0'
CASE = '24x40-holes'


@pytest.mark.parametrize('term', ('ssim', 'tv'))
def test_forward_and_backward_replay_in_a_graph(term):
    H, W, mask, pred, gt, occ = T.inputs(CASE, term)
    L = _abi.lib()
    n = pred.shape[0]
    w = T.WINDOW if term == 'ssim' else 1
    nbytes = L.invr_imgloss_workspace_bytes(H, W, w)
    ws = T.aligned_bytes(nbytes, 0xFF)
    taps = R.gaussian_taps(w).to(DEV)
    mask_d, occ_d = mask.to(DEV), occ.to(DEV)
    pred_d, gt_d = torch.zeros(n, 3, device=DEV), torch.zeros(n, 3, device=DEV)
    out8, g_rgb = torch.zeros(8, device=DEV), torch.zeros(n, 3, device=DEV)
    gl = torch.tensor([T.G_LOSS], device=DEV)
    p, pw, pm = _abi.ptr, (_abi.ptr(ws, torch.uint8), nbytes), _abi.ptr(mask_d, torch.uint8)

    def calls():
        if term == 'ssim':
            _abi.check(L.invr_ssim_fwd(p(pred_d), p(gt_d), pm, p(taps), w, n, H, W, *pw, p(out8), _abi.stream_ptr()))
            _abi.check(L.invr_ssim_bwd(pm, p(taps), w, n, H, W, *pw, p(gl), p(g_rgb), _abi.stream_ptr()))
        else:
            _abi.check(L.invr_tv_fwd(p(pred_d), p(gt_d), p(occ_d, torch.uint8), pm, n, H, W, *pw, p(out8), _abi.stream_ptr()))
            _abi.check(L.invr_tv_bwd(pm, n, H, W, *pw, p(gl), p(g_rgb), _abi.stream_ptr()))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        calls()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode='thread_local'):
        calls()
    pred_d.copy_(pred.to(DEV))                          # the values arrive after the capture
    gt_d.copy_(gt.to(DEV))
    ref = T.run(term, CASE, T.DEV)
    for _ in range(2):
        ws.fill_(0x5A)
        out8.fill_(float('nan'))
        g_rgb.fill_(float('nan'))
        g.replay()
        torch.cuda.synchronize()
        assert T.same_bits(out8.cpu(), ref['out8']) and T.same_bits(g_rgb.cpu(), ref['g_rgb'])
