"""GPU: the SSIM and TV image terms' kernels (csrc/k_imgloss.hip) through the C ABI of include/invr_imgloss.h.

Every stored map (the assembled images and ranks exactly; the five filtered maps, S, the gradient of the assembled image), out8 and
g_rgb per ray are compared element by element with the float64 statement of tests/imgloss_reference.py.  The bound of each comparison
is that module's running error analysis of an fp32 evaluation of the same formula from the same fp32 inputs (derived, not fitted: see
its docstring); each case prints the worst ratio error / bound.  The objective's twins are held bit for bit to invr_train_loss_fwd /
_bwd on the same `terms`, their loss to the stated fp32 sum.

Outputs and the workspace are pre-filled: NaN bytes where a kernel must write, a marker where it must not.
tests/test_hostsim_imgloss_cpu.py runs the same bodies on the CPU wave machine."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import imgloss_reference as R             # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
MARK = -0x365A5A5B                                   # int32 bit pattern of a float no kernel may produce here
G_LOSS = 0.7
WINDOW = 11

SHAPES = ((2, 2), (7, 9), (11, 11), (16, 16), (24, 40), (64, 64))
MASKS = ('full', 'holes', 'one', 'none')
CASES = ['%dx%d-%s' % (h, w, m) for h, w in SHAPES for m in MASKS]
WINDOW_CASES = (('24x40-holes', 1), ('24x40-holes', 5), ('17x33-holes', 31), ('7x9-full', 31))          # the halo at its ends
TV_OCC = ('p70', 'nothing', 'lastrow', 'lastcol')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'imgloss_small.npz')


def parse(case):
    hw, m = case.split('-')
    h, w = hw.split('x')
    return int(h), int(w), m


@functools.lru_cache(maxsize=None)
def inputs(case, term='ssim', occ='p70'):
    """-> H, W, mask (H*W uint8), pred (n, 3), gt (n, 3), occupancy (n uint8): fp32 CPU tensors, seeded by the case.  SSIM: the target is
    the prediction + N(0, 0.1^2); TV: a dark target under a prediction that spans [0, 1] (about half of the relu terms active)."""
    H, W, m = parse(case)
    g = torch.Generator().manual_seed(H * 10007 + W * 101 + MASKS.index(m) * 7)
    if m == 'full':
        mask = torch.ones(H * W, dtype=torch.uint8)
    elif m == 'holes':
        mask = (torch.rand(H * W, generator=g) < 0.8).to(torch.uint8)
    elif m == 'one':
        mask = torch.zeros(H * W, dtype=torch.uint8)
        mask[int(torch.randint(0, H * W, (1,), generator=g))] = 1
    else:
        mask = torch.zeros(H * W, dtype=torch.uint8)
    n = int(mask.sum())
    if term == 'ssim':
        pred = torch.rand(n, 3, generator=g)
        gt = (pred + torch.randn(n, 3, generator=g) * 0.1).clamp(0.0, 1.0)
    else:
        pred, gt = torch.rand(n, 3, generator=g), 0.3 * torch.rand(n, 3, generator=g)
    pix = torch.nonzero(mask).reshape(-1)
    if occ == 'p70':
        o = torch.rand(n, generator=g) < 0.7
    elif occ == 'nothing':
        o = torch.zeros(n, dtype=torch.bool)
    elif occ == 'lastrow':
        o = pix // W == H - 1
    else:
        o = pix % W == W - 1
    return H, W, mask, pred, gt, o.to(torch.uint8)


def golden_inputs(name, term):
    z = np.load(GOLDEN)
    H, W = (int(v) for v in name.split('x'))
    t = lambda k: torch.from_numpy(z['%s/%s' % (name, k)])
    return H, W, t('mask'), t(term + '_pred'), t(term + '_gt'), t('occ'), z


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def aligned_bytes(nbytes, fill):
    raw = torch.empty(nbytes + 256, dtype=torch.uint8, device=DEV)
    off = (-raw.data_ptr()) % 256
    t = raw[off:off + nbytes]
    t.fill_(fill)
    return t


def guarded(rows, cols=None):
    """(rows [, cols]) of NaN followed by 4 marker rows, on DEV"""
    shape = (rows + 4,) if cols is None else (rows + 4, cols)
    t = torch.full(shape, MARK, dtype=torch.int32).view(torch.float32).clone()
    t[:rows] = float('nan')
    return t.to(DEV)


def unguard(t, rows, what):
    t = t.cpu()
    assert (t[rows:].contiguous().view(torch.int32) == MARK).all(), 'written past ' + what
    return t[:rows]


TERMS = torch.tensor([3.25, 40.0, 0.625, 7.0, 0.0, 0.0, 0.0, 0.0])          # offset sum / rows, pair sum / rows
WEIGHTS = (10.0, 0.1, 0.1, 1)                                                   # w_pair, w_dist, w_off, use_pair


def run_raw(term, H, W, mask, pred, gt, occ, window=WINDOW, fill=0xFF, g_loss=G_LOSS, twin=False):
    """One forward + backward of a term (or of the objective's twin around it) over a fresh workspace of `fill` bytes -> dict of CPU
    tensors: every workspace view, out8, g_rgb (n, 3) and, for a twin, err, g_dist, g_terms."""
    L = _abi.lib()
    n = pred.shape[0]
    w = window if term == 'ssim' else 1
    nbytes = L.invr_imgloss_workspace_bytes(H, W, w)
    assert nbytes > 0
    ws = aligned_bytes(nbytes, fill)
    out8, g_rgb = guarded(8), guarded(n, 3)
    mask_d, pred_d, gt_d, occ_d = mask.to(DEV), pred.contiguous().to(DEV), gt.contiguous().to(DEV), occ.to(DEV)
    taps = R.gaussian_taps(w).to(DEV)
    gl = torch.tensor([g_loss], dtype=torch.float32, device=DEV)
    p, pw, pm = _abi.ptr, (_abi.ptr(ws, torch.uint8), nbytes), _abi.ptr(mask_d, torch.uint8)
    r = {}
    if twin:
        g = torch.Generator().manual_seed(n + 1)
        dist = torch.rand(n, generator=g).to(DEV)
        terms = TERMS.to(DEV)
        err, g_dist, g_terms = guarded(n), guarded(n), guarded(8)
        obj = (n, H, W) + WEIGHTS + pw
        if term == 'ssim':
            _abi.check(L.invr_train_loss_ssim_fwd(p(pred_d), p(gt_d), pm, p(taps), w, p(dist), p(terms), *obj, p(out8), p(err), _abi.stream_ptr()))
            _abi.check(L.invr_train_loss_ssim_bwd(pm, p(taps), w, p(terms), *obj, p(gl), p(g_rgb), p(g_dist), p(g_terms), _abi.stream_ptr()))
        else:
            _abi.check(L.invr_train_loss_tv_fwd(p(pred_d), p(gt_d), p(occ_d, torch.uint8), pm, p(dist), p(terms), *obj, p(out8), p(err),
                                                _abi.stream_ptr()))
            _abi.check(L.invr_train_loss_tv_bwd(pm, p(terms), *obj, p(gl), p(g_rgb), p(g_dist), p(g_terms), _abi.stream_ptr()))
        # the plain objective on the same inputs
        o_out, o_err, o_rgb, o_dist, o_terms = guarded(8), guarded(n), guarded(n, 3), guarded(n), guarded(8)
        nz = lambda t: t if t.numel() else torch.zeros((1,) + tuple(t.shape[1:]), device=DEV)          # (it takes no NULL, even for no rays)
        _abi.check(L.invr_train_loss_fwd(p(nz(pred_d)), p(nz(gt_d)), p(nz(dist)), p(terms), n, *WEIGHTS, p(o_out), p(o_err), _abi.stream_ptr()))
        _abi.check(L.invr_train_loss_bwd(p(nz(pred_d)), p(nz(gt_d)), p(terms), n, *WEIGHTS, p(gl), p(o_rgb), p(o_dist), p(o_terms), _abi.stream_ptr()))
        sync()
        r.update(err=unguard(err, n, 'err'), g_dist=unguard(g_dist, n, 'g_dist'), g_terms=unguard(g_terms, 8, 'g_terms'),
                 plain={'out8': unguard(o_out, 8, 'out8'), 'err': unguard(o_err, n, 'err'), 'g_rgb': unguard(o_rgb, n, 'g_rgb'),
                        'g_dist': unguard(o_dist, n, 'g_dist'), 'g_terms': unguard(o_terms, 8, 'g_terms')})
    elif term == 'ssim':
        _abi.check(L.invr_ssim_fwd(p(pred_d), p(gt_d), pm, p(taps), w, n, H, W, *pw, p(out8), _abi.stream_ptr()))
        _abi.check(L.invr_ssim_bwd(pm, p(taps), w, n, H, W, *pw, p(gl), p(g_rgb), _abi.stream_ptr()))
    else:
        _abi.check(L.invr_tv_fwd(p(pred_d), p(gt_d), p(occ_d, torch.uint8), pm, n, H, W, *pw, p(out8), _abi.stream_ptr()))
        _abi.check(L.invr_tv_bwd(pm, n, H, W, *pw, p(gl), p(g_rgb), _abi.stream_ptr()))
    sync()
    v = _abi.imgloss_views(ws, H, W, w)
    lay = v.pop('layout')
    r.update({k: t.cpu().clone() for k, t in v.items()})
    r['n_ssim'], r['n_tv'] = lay.n_ssim, lay.n_tv
    r['out8'], r['g_rgb'] = unguard(out8, 8, 'out8'), unguard(g_rgb, n, 'g_rgb')
    return r


@functools.lru_cache(maxsize=None)
def run(term, case, dev, occ='p70', window=WINDOW, twin=False):
    return run_raw(term, *inputs(case, term, occ), window=window, twin=twin)


@functools.lru_cache(maxsize=None)
def exact(term, case, occ='p70', window=WINDOW, scale=1.0):
    """the float64 statement with its bounds, computed once per case"""
    H, W, mask, pred, gt, o = inputs(case, term, occ)
    ip, ig = R.assemble(pred, mask, H, W), R.assemble(gt, mask, H, W)
    if term == 'ssim':
        return R.ssim(ip, ig, R.gaussian_taps(window), np.float32(G_LOSS), scale)
    return R.tv(ip, ig, R.assemble(o[:, None], mask, H, W)[0] != 0, np.float32(G_LOSS), scale)


def bits(t):
    return t.contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def check_assembly(r, H, W, mask, pred, gt):
    assert same_bits(r['img'][0], R.assemble(pred, mask, H, W)) and same_bits(r['img'][1], R.assemble(gt, mask, H, W))
    rank = torch.full((H * W,), -1, dtype=torch.int32)
    rank[mask.bool()] = torch.arange(pred.shape[0], dtype=torch.int32)
    assert torch.equal(r['rank'].reshape(-1), rank)


def held(e, got, what, case, report):
    ok, ratio = e.holds(got)
    report.append('%s %.3f' % (what, ratio))
    assert ok, (case, what, ratio)


# ---- SSIM -------------------------------------------------------------------------------------------------------------------------------
def ssim_body(case, window, r, ex):
    H, W, mask, pred, gt, _ = inputs(case, 'ssim')
    rep = []
    check_assembly(r, H, W, mask, pred, gt)
    for j, name in enumerate(('mu1', 'mu2', 'e11', 'e22', 'e12')):
        held(ex['mom'][j], r['mom'][j], name, case, rep)
    held(ex['S'], r['smap'], 'S', case, rep)
    held(ex['ssim'], r['out8'][0], 'ssim', case, rep)
    assert same_bits(r['out8'][1:2], 1.0 - r['out8'][0:1]) and (bits(r['out8'][2:]) == 0).all()
    # the mean: the float64 sum of the stored S over the workgroups' partials, rounded to fp32 once
    assert abs(float(r['partial'][:r['n_ssim']].sum()) - float(r['smap'].double().sum())) <= 2.0 ** -40 * r['smap'].numel()
    assert abs(float(r['out8'][0]) - float(r['smap'].double().mean())) <= 2.0 ** -24 * abs(float(r['smap'].double().mean())) + 2.0 ** -40
    # layer-local, the tighter statement: S, p, q, r from the kernel's OWN stored moments, the gradient from its own stored p, q, r
    S, p, q, rr = R.ssim_maps([R.E.exact(r['mom'][j]) for j in range(5)])
    for e, got, name in ((S, r['smap'], 'S|mom'), (p, r['pqr'][0], 'p|mom'), (q, r['pqr'][1], 'q|mom'), (rr, r['pqr'][2], 'r|mom')):
        held(e, got, name, case, rep)
    if pred.shape[0]:
        held(ex['gimg'], r['gimg'], 'gimg', case, rep)
        local = R.ssim_grad(R.E.exact(r['img'][0]), R.E.exact(r['img'][1]), *(R.E.exact(r['pqr'][j]) for j in range(3)), R.gaussian_taps(window),
                            np.float32(G_LOSS))
        held(local, r['gimg'], 'gimg|pqr', case, rep)
        assert same_bits(r['g_rgb'], R.rays(r['gimg'], mask).contiguous())          # masked-out pixels' gradients are dropped
    print('ssim %-14s w %2d  error / bound: %s' % (case, window, '  '.join(rep)))


@pytest.mark.parametrize('case', CASES)
def test_ssim_against_float64(case):
    ssim_body(case, WINDOW, run('ssim', case, DEV), exact('ssim', case))


@pytest.mark.parametrize('case,window', WINDOW_CASES)
def test_ssim_other_windows(case, window):
    ssim_body(case, window, run('ssim', case, DEV, window=window), exact('ssim', case, window=window))


# ---- TV -----------------------------------------------------------------------------------------------------------------------------------
def tv_body(case, occ, r, ex):
    H, W, mask, pred, gt, o = inputs(case, 'tv', occ)
    rep = []
    check_assembly(r, H, W, mask, pred, gt)
    mask_gt = R.assemble(o[:, None], mask, H, W)[0] != 0
    assert torch.equal(r['occ'] != 0, mask_gt)
    out = r['out8']
    held(ex['eps_x'], out[3], 'eps_x', case, rep)
    held(ex['eps_y'], out[4], 'eps_y', case, rep)
    assert float(out[5]) == ex['k_x'] == float(mask_gt[:-1, :].sum()) and float(out[6]) == ex['k_y'] == float(mask_gt[:, :-1].sum())
    held(ex['mean_x'], out[1], 'mean_x', case, rep)
    held(ex['mean_y'], out[2], 'mean_y', case, rep)
    held(ex['tv'], out[0], 'tv', case, rep)
    assert bits(out[7:])[0] == 0
    assert bool(torch.isnan(out[0])) == (ex['k_x'] == 0 or ex['k_y'] == 0)          # the mean of an empty selection, as in the reference
    if pred.shape[0]:
        held(ex['gimg'], r['gimg'], 'gimg', case, rep)
        assert torch.isfinite(r['gimg']).all()                                      # an empty selection contributes nothing
        assert same_bits(r['g_rgb'], R.rays(r['gimg'], mask).contiguous())
    print('tv   %-14s %-8s error / bound: %s' % (case, occ, '  '.join(rep)))


@pytest.mark.parametrize('case', CASES)
def test_tv_against_float64(case):
    tv_body(case, 'p70', run('tv', case, DEV), exact('tv', case))


@pytest.mark.parametrize('occ', TV_OCC[1:])
@pytest.mark.parametrize('case', ('2x2-full', '7x9-holes', '16x16-full', '24x40-holes'))
def test_tv_empty_and_edge_selections(case, occ):
    """an occupancy that selects nothing, and ones inside the last row / column only: those pixels are in neither selection's first
    operand along that axis (k = 0 there: NaN), and only in the other axis' selection"""
    r, ex = run('tv', case, DEV, occ=occ), exact('tv', case, occ=occ)
    tv_body(case, occ, r, ex)
    assert torch.isnan(r['out8'][0])
    if occ == 'lastrow':
        assert float(r['out8'][5]) == 0 and torch.isnan(r['out8'][1])
    if occ == 'lastcol':
        assert float(r['out8'][6]) == 0 and torch.isnan(r['out8'][2])
    if occ == 'nothing' and r['g_rgb'].numel():
        assert (bits(r['g_rgb']) & 0x7fffffff == 0).all()


# ---- the golden cases of the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ('7x9', '16x16', '24x40'))
@pytest.mark.parametrize('term', ('ssim', 'tv'))
def test_golden_cases(term, name):
    """the reference's own inputs: value and gradient against its float64 evaluation, inside the derived bound"""
    H, W, mask, pred, gt, occ, z = golden_inputs(name, term)
    r = run_raw(term, H, W, mask, pred, gt, occ, g_loss=1.0)
    ip, ig = R.assemble(pred, mask, H, W), R.assemble(gt, mask, H, W)
    ex = R.ssim(ip, ig, R.gaussian_taps(11)) if term == 'ssim' else R.tv(ip, ig, R.assemble(occ[:, None], mask, H, W)[0] != 0)
    v64, g64 = float(z['%s/%s_f64' % (name, term)]), torch.from_numpy(z['%s/%s_grad_f64' % (name, term)])
    dv, dg = abs(float(r['out8'][0]) - v64), (r['g_rgb'].double() - g64).abs()
    bound_g = R.rays(ex['gimg'].e, mask)
    print('%s golden %s: |value - float64| %.3g (bound %.3g, reference fp32 %.3g)   max |grad - float64| %.3g (bound %.3g, reference fp32 %.3g)'
          % (term, name, dv, float(ex[term].e), abs(float(z['%s/%s_f32' % (name, term)]) - v64), float(dg.max()), float(bound_g.max()),
             float(np.abs(z['%s/%s_grad_f32' % (name, term)] - g64.numpy()).max())))
    assert dv <= float(ex[term].e) and bool((dg <= bound_g + R.TINY).all())


# ---- determinism, the objective's twins, the arguments ----------------------------------------------------------------------------------
@pytest.mark.parametrize('term', ('ssim', 'tv'))
@pytest.mark.parametrize('case', ('7x9-holes', '24x40-holes', '64x64-full'))
def test_two_runs_over_dirty_workspaces_are_bit_identical(term, case):
    a = run(term, case, DEV)
    b = run_raw(term, *inputs(case, term), fill=0x5A)
    own = ('rank', 'img', 'out8', 'gimg', 'g_rgb') + (('mom', 'smap', 'pqr') if term == 'ssim' else ('occ', 'tvmax'))
    for k in own:
        assert same_bits(a[k], b[k]), k
    n = a['n_ssim'] if term == 'ssim' else 4 * a['n_tv']
    assert same_bits(a['partial'][:n], b['partial'][:n])


@pytest.mark.parametrize('term', ('ssim', 'tv'))
@pytest.mark.parametrize('case', ('2x2-full', '7x9-holes', '24x40-holes', '64x64-holes', '16x16-none'))
def test_objective_twins(term, case):
    H, W, mask, pred, gt, o = inputs(case, term)
    r, alone = run(term, case, DEV, twin=True), run(term, case, DEV)
    pl = r['plain']
    # the regulariser outputs, the statistics and err: invr_train_loss_fwd's on the same terms, bit for bit
    assert same_bits(r['out8'][1:6], pl['out8'][1:6]) and same_bits(r['err'], pl['err'])
    assert same_bits(r['g_dist'], pl['g_dist']) and same_bits(r['g_terms'], pl['g_terms'])
    f = lambda v: torch.tensor(v, dtype=torch.float32)
    t = (f(1.0) - alone['out8'][0]) if term == 'ssim' else alone['out8'][0]
    assert (same_bits(r['out8'][6:7], t.reshape(1)) or bool(torch.isnan(t) and torch.isnan(r['out8'][6]))) and bits(r['out8'][7:])[0] == 0
    img, rd, off, pair = pl['out8'][1], pl['out8'][3], pl['out8'][4], pl['out8'][5]
    loss = f(0.0) + f(WEIGHTS[0]) * pair
    loss = loss + f(WEIGHTS[1]) * rd
    loss = loss + f(WEIGHTS[2]) * off
    loss = loss + (f(0.1 if term == 'ssim' else 0.01) * t + img)          # the reference's order: loss += (w t + img_loss)
    if torch.isnan(loss):
        assert torch.isnan(r['out8'][0])
    else:
        assert same_bits(r['out8'][0:1], loss.reshape(1)), (float(r['out8'][0]), float(loss))
    if pred.shape[0]:
        # g_rgb = the MSE's gradient (invr_train_loss_bwd's, one rounding each) + the term's with its weight
        ex = exact(term, case, scale=-0.1 if term == 'ssim' else 0.01)
        term_g = R.E(R.rays(ex['gimg'].v, mask), R.rays(ex['gimg'].e, mask))
        total = R.E(pl['g_rgb'].double() + term_g.v, term_g.e + R.U * (pl['g_rgb'].double().abs() + term_g.v.abs() + term_g.e))
        ok, ratio = total.holds(r['g_rgb'])
        print('%s twin %-14s g_rgb error / bound %.3f' % (term, case, ratio))
        assert ok, ratio


def test_mask_bits_beyond_n_rays_are_ignored():
    H, W, mask, pred, gt, o = inputs('7x9-holes', 'tv')
    n = pred.shape[0] - 5
    for term in ('ssim', 'tv'):
        r = run_raw(term, H, W, mask, pred[:n].clone(), gt[:n].clone(), o[:n].clone())
        rank = r['rank'].reshape(-1)
        assert int((rank >= 0).sum()) == n and int(rank.max()) == n - 1
        assert torch.isfinite(r['g_rgb']).all()


@pytest.mark.parametrize('hw', ((2, 2), (7, 9), (16, 16)))
def test_no_rays(hw):
    H, W = hw
    z = torch.zeros(0, 3)
    r = run_raw('ssim', H, W, torch.zeros(H * W, dtype=torch.uint8), z, z, torch.zeros(0, dtype=torch.uint8))
    assert float(r['out8'][0]) == 1.0 and float(r['out8'][1]) == 0.0          # two black images
    assert r['g_rgb'].numel() == 0 and (r['rank'] == -1).all() and (bits(r['img']) == 0).all()
    r = run_raw('tv', H, W, torch.zeros(H * W, dtype=torch.uint8), z, z, torch.zeros(0, dtype=torch.uint8))
    assert torch.isnan(r['out8'][0]) and r['g_rgb'].numel() == 0


def test_argument_checks_launch_nothing():
    L = _abi.lib()
    assert L.invr_imgloss_workspace_bytes(1, 8, 11) == 0 and L.invr_imgloss_workspace_bytes(8, 2049, 11) == 0
    assert L.invr_imgloss_workspace_bytes(8, 8, 10) == 0 and L.invr_imgloss_workspace_bytes(8, 8, 33) == 0
    ws = aligned_bytes(L.invr_imgloss_workspace_bytes(8, 8, 11), 0xFF)
    z = torch.zeros(64, 3, device=DEV)
    m = torch.ones(64, dtype=torch.uint8, device=DEV)
    o = torch.zeros(8, device=DEV)
    taps = R.gaussian_taps(11).to(DEV)
    args = lambda H, W, n, w, nbytes: (_abi.ptr(z), _abi.ptr(z), _abi.ptr(m, torch.uint8), _abi.ptr(taps), w, n, H, W, _abi.ptr(ws, torch.uint8),
                                       nbytes, _abi.ptr(o), _abi.stream_ptr())
    assert L.invr_ssim_fwd(*args(1, 8, 8, 11, ws.numel())) != 0 and b'H, W must be in' in L.invr_last_error()
    assert L.invr_ssim_fwd(*args(8, 8, 64, 12, ws.numel())) != 0 and b'window' in L.invr_last_error()
    assert L.invr_ssim_fwd(*args(8, 8, 65, 11, ws.numel())) != 0 and b'n_rays' in L.invr_last_error()
    assert L.invr_ssim_fwd(*args(8, 8, 64, 11, ws.numel() - 1)) != 0 and b'workspace too small' in L.invr_last_error()
    assert L.invr_tv_fwd(_abi.ptr(z), _abi.ptr(z), _abi.ptr(m, torch.uint8), _abi.ptr(m, torch.uint8), 64, 8, 8, _abi.ptr(ws, torch.uint8),
                         ws.numel() - 1, _abi.ptr(o), _abi.stream_ptr()) != 0 and b'workspace too small' in L.invr_last_error()
    sync()
    assert (ws == 0xFF).all()
