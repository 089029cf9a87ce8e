"""GPU: the geometry-map kernels (csrc/k_geomaps.hip) through the C ABI of include/invr_geomaps.h against the float64 restatement of the
contract (tests/geomaps_reference.py), the depth pass behind a render against the dense form bit for bit, and the host layer
(invr.geomaps.geometry_maps, Renderer.render with cfg.render_depth).

Bounds (u = 2^-24, the unit round-off of fp32):
  depth_map   epsilon 0: |got - sum_i w_i z_i| <= (2 S + 4) u sum_i w_i z_i, the sum in float64 over the fp32 weights invr_composite_fwd
              returns for the same occupancies and the fp32 depths (two rounding chains of length S; every term is non-negative).
              epsilon 1: invr_composite_fwd composites with epsilon 0 only, so the weights are the float64 product of the fp32
              occupancies and the bound is (2 S + 24) u: a factor fl(fl(1 - a) + 1) carries 2 u, a weight the factors in front of it
              (2 S u) and at most 6 + 3 + 2 multiplications of the scan, the passes' running product and the weight itself; the sum
              adds one fmaf per pass (3) and the 6 additions of the wave sum; 2 u for the two conversions of the comparison.  2^S
              overflows fp32 from S = 128 on (as the render's own weights do): where the float64 transmittance passes 2^126 the
              fp32 result may be anything non-finite and is compared no further.
  surf_depth  8 u max(|z_{i-1}|, |z_i|) (3 roundings in t, 3 in the lerp, a margin), and between the two sample depths up to that.
  stencil     u (2 (|o| + |z d|) + |x| + h) per coordinate: the fmaf rounds once (|x| u), the addition of h once more.
  normals     6 u per component, 4 u on the length.

Outputs are pre-filled: NaN bytes where a kernel must write, a marker where it must not.  tests/test_hostsim_geomaps_cpu.py runs
checks 1 to 4 on the CPU wave machine."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import geomaps_reference as R             # noqa: E402  (checker only)
from invr import _abi                                # noqa: E402

DEV = 'cuda:0'
RES = 64                                             # the frame of check 2 (tests/test_hostsim_geomaps_cpu.py cuts it)
MARK = -0x365A5A5B                                   # int32 bit pattern no kernel produces here
UNSET = -2                                           # surf_index before the call (-1, the NaN bytes, is a result)
U = 2.0 ** -24
LEVEL = 0.5

SHAPES = [(1, 2), (5, 8), (9, 64), (17, 128), (37, 100), (3, 192)]


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def prefilled(n, written, dtype=torch.float32, fill=-1):
    """(n,) on DEV: `fill` (default: NaN bytes) in the first `written` entries, MARK behind them."""
    t = torch.full((n,), MARK, dtype=torch.int32)
    t[:written] = fill
    return t.view(dtype).to(DEV)


# ---- 1. dense depth ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(R_, S):
    """-> (occ (R_ + crafted, S) fp32, near, far): random rows in [0, 1] with about 80 % exact zeros, then the crafted rows."""
    g = np.random.RandomState(1000 * R_ + S)
    occ = g.uniform(0.0, 1.0, (R_, S)).astype(np.float32)
    occ[g.uniform(size=occ.shape) < 0.8] = 0.0
    low = lambda: g.uniform(0.0, 0.45, S).astype(np.float32)
    crafted = []
    crafted.append(np.zeros(S, np.float32))                                   # all zeros
    r = low(); r[0] = 1.0; crafted.append(r)                                  # occ_0 = 1
    r = low(); r[S // 2] = np.float32(LEVEL); crafted.append(r)               # a value exactly on the level counts
    r = low(); r[-1] = 0.9; crafted.append(r)                                 # the first crossing at the last sample
    r = np.zeros(S, np.float32); r[(2 * S) // 3:] = 0.7; crafted.append(r)    # a crossing preceded only by zeros
    r = low(); r[-1] = 0.8; r[0] = np.nan; crafted.append(r)                  # a NaN before the crossing ...
    r = low(); r[-1] = 0.8; r[-2] = np.nan; crafted.append(r)                 # ... and right in front of it (interpolates as 0)
    if S > 64:
        r = np.zeros(S, np.float32); r[64] = 0.75; crafted.append(r)          # a crossing at the first sample of a pass behind an empty one
        r = low(); r[63] = 0.2; r[64] = 0.6; r[:63] = 0.0; crafted.append(r)  # ... whose sample in front lies in the pass before
    occ = np.concatenate([occ, np.stack(crafted)], 0)
    near = g.uniform(1.0, 2.0, occ.shape[0]).astype(np.float32)
    far = (near + g.uniform(1.0, 2.0, occ.shape[0])).astype(np.float32)
    return occ, near, far


def depth_fwd(occ, near, far, z_vals, eps, level=LEVEL, outputs=(True, True, True)):
    """invr_depth_fwd over prefilled outputs -> (depth_map, surf_index, surf_depth) CPU tensors (None where not asked for); entries
    behind n_rays are asserted to keep their marker."""
    L = _abi.lib()
    n, S = occ.shape
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    occ_d, near_d, far_d, z_d = dev(occ), dev(near), dev(far), dev(z_vals)
    dm = prefilled(n + 3, n) if outputs[0] else None
    si = prefilled(n + 3, n, torch.int32, UNSET) if outputs[1] else None
    sd = prefilled(n + 3, n) if outputs[2] else None
    _abi.check(L.invr_depth_fwd(_abi.ptr(occ_d), _abi.ptr(near_d), _abi.ptr(far_d), _abi.ptr(z_d), n, S, float(eps), float(level),
                                _abi.ptr(dm), _abi.ptr(si, torch.int32), _abi.ptr(sd), _abi.stream_ptr()))
    sync()
    res = []
    for t in (dm, si, sd):
        if t is None:
            res.append(None)
            continue
        t = t.cpu()
        assert (bits(t[n:]) == MARK).all(), 'written behind the last ray'
        res.append(t[:n])
    return res


def composite_weights(occ):
    """the fp32 weights invr_composite_fwd (epsilon 0) returns for these occupancies"""
    n, S = occ.shape
    raw = torch.zeros(n, S, 4)
    raw[:, :, 3] = torch.from_numpy(occ)
    raw = raw.to(DEV)
    w, rgb, acc = torch.empty(n, S, device=DEV), torch.empty(n, 3, device=DEV), torch.empty(n, device=DEV)
    _abi.check(_abi.lib().invr_composite_fwd(_abi.ptr(raw), n, S, _abi.ptr(w), _abi.ptr(rgb), _abi.ptr(acc), _abi.stream_ptr()))
    sync()
    return w.cpu().numpy()


def check_dense(occ, z, eps, got):
    dm, si, sd = got
    n, S = occ.shape
    idx, depth, lo, hi = R.first_crossing(occ, z, LEVEL)
    assert np.array_equal(si.numpy(), idx), 'surf_index'
    # depth_map
    if eps == 0:
        want = R.depth64(composite_weights(occ), z)
        bound, finite = (2 * S + 4) * U * want, np.isfinite(want)
    else:
        with np.errstate(invalid='ignore', over='ignore'):
            want = R.depth64(R.weights64(occ, eps), z)
            T = np.cumprod(1.0 - np.nan_to_num(occ.astype(np.float64)) + eps, axis=1)[:, :-1].max(1)      # the transmittance of the last sample
        bound, finite = (2 * S + 24) * U * want, np.isfinite(want) & (T < 2.0 ** 126)
        over = np.isfinite(want) & (T >= 2.0 ** 128)
        assert not np.isfinite(dm.numpy()[over]).any(), 'a transmittance beyond fp32 gave a finite depth'
    g = dm.numpy().astype(np.float64)
    nan_rows = np.isnan(want)
    assert np.isnan(g[nan_rows]).all() and nan_rows.sum() <= 2          # (the two crafted NaN rows, where the NaN weighs in)
    err = np.abs(g[finite] - want[finite])
    print('depth_map (%d, %d) eps %g: max error / bound = %.3f over %d rows' % (n, S, eps, float((err / np.maximum(bound[finite], 1e-300)).max(initial=0.0)), finite.sum()))
    assert (err <= bound[finite]).all()
    zero = finite & (want == 0)
    assert (zero.any() or eps != 0) and (bits(dm)[torch.from_numpy(zero)] == 0).all(), 'a zero sum is +0'
    # surf_depth
    b = 8 * U * np.maximum(np.abs(lo), np.abs(hi))
    s = sd.numpy().astype(np.float64)
    assert np.isfinite(s).all()
    print('surf_depth: max error / bound = %.3f, %d crossings' % (float((np.abs(s - depth)[idx >= 0] / b[idx >= 0]).max()), (idx >= 0).sum()))
    assert (np.abs(s - depth) <= b).all()
    assert (s >= lo - b).all() and (s <= hi + b).all()
    assert (bits(sd)[torch.from_numpy(idx < 0)] == 0).all(), 'no crossing: +0'
    assert (idx == 0).any() and (idx < 0).any() and (idx == S - 1).any()


@pytest.mark.parametrize('eps', [0.0, 1.0])
@pytest.mark.parametrize('shape', SHAPES)
def test_dense_depth_and_first_crossing(shape, eps):
    occ, near, far = dense_case(*shape)
    z = R.z_vals_f32(near, far, shape[1])
    check_dense(occ, z, eps, depth_fwd(occ, near, far, None, eps))


@pytest.mark.parametrize('shape', [(5, 8), (37, 100), (17, 128)])
def test_dense_depth_from_a_jittered_z_vals_pointer(shape):
    from oracle import nvr_oracle as O               # checker only: the stratified depths by the oracle's formula
    occ, near, far = dense_case(*shape)
    n, S = occ.shape
    g = torch.Generator().manual_seed(S)
    jit = torch.rand(1, n, S, generator=g)
    o = torch.zeros(1, n, 3)
    _, z = O.sample_points(o, o, torch.from_numpy(near)[None], torch.from_numpy(far)[None], S, jitter=jit)
    z = z[0].to(torch.float32).numpy()
    assert (np.diff(z, axis=1) >= 0).all() and not np.array_equal(z, R.z_vals_f32(near, far, S))
    check_dense(occ, z, 0.0, depth_fwd(occ, None, None, z, 0.0))


def test_any_dense_output_may_be_null():
    occ, near, far = dense_case(5, 8)
    full = depth_fwd(occ, near, far, None, 0.0)
    for k in range(3):
        only = depth_fwd(occ, near, far, None, 0.0, outputs=tuple(i == k for i in range(3)))
        assert [o is not None for o in only] == [i == k for i in range(3)]
        assert torch.equal(bits(only[k]), bits(full[k]))


# ---- 2. the merged source (the depth pass behind a render) equals the dense source, bit for bit ----------------------------------
_NETS, _FRAMES = {}, {}


def net_of(S, **kw):
    key = (DEV, S, tuple(sorted(kw.items())))
    if key not in _NETS:
        import invr  # noqa: F401
        from invr import params
        from invr.config import make_cfg
        from invr.network import Network
        cfg = make_cfg(table_log2=8, N_samples=S, eval_vertex_rows=0, **kw)          # (no de-hashed vertex tables: each net would build its own)
        net = Network(cfg=cfg)
        net.load_state_dict(params.init_state_dict(cfg, seed=4), strict=True)
        _NETS[key] = net.to(DEV).eval()
    return _NETS[key]


def frame(res):
    """-> (batch on DEV, (ray_o, ray_d, near, far))"""
    if (DEV, res) not in _FRAMES:
        from invr import scene
        b, _ = scene.make_scene(H=res, W=res)
        b = {k: v.to(DEV) for k, v in scene.to_torch(b).items()}
        _FRAMES[(DEV, res)] = (b, tuple(b[k][0].contiguous() for k in ('ray_o', 'ray_d', 'near', 'far')))
    return _FRAMES[(DEV, res)]


def abi_render(net, S, res, geo, max_active=0, level=LEVEL):
    """invr_render_fwd (geo False, occ NULL) or invr_render_fwd_geo (occ and the three maps) of the frame -> dict of device tensors"""
    L = _abi.lib()
    b, (ro, rd, near, far) = frame(res)
    ctx = net.prepare(b)
    n = ro.shape[0]
    o = {'rgb_map': torch.empty(n, 3, device=DEV), 'acc_map': torch.empty(n, device=DEV), 'raw': torch.empty(n * S, 4, device=DEV),
         'stats': torch.zeros(_abi.STATS_LEN, dtype=torch.int32, device=DEV)}
    if geo:
        o['occ'] = torch.empty(n, S, device=DEV)
        o['depth_map'], o['surf_depth'] = prefilled(n + 3, n), prefilled(n + 3, n)
        o['surf_index'] = prefilled(n + 3, n, torch.int32, UNSET)
    net._ws = None
    nbytes = L.invr_workspace_bytes(n, S, max_active)
    ws = net.workspace(nbytes, ro.device)
    args = (C.byref(ctx.scene), C.byref(ctx.model), _abi.ptr(ro), _abi.ptr(rd), _abi.ptr(near), _abi.ptr(far), _abi.ptr(None), n, S,
            _abi.ptr(o['rgb_map']), _abi.ptr(o['acc_map']), _abi.ptr(o['raw']), _abi.ptr(o.get('occ')), _abi.ptr(None), _abi.ptr(None),
            _abi.ptr(o['stats'], torch.int32), C.c_void_p(ws.data_ptr()), nbytes, max_active, _abi.stream_ptr())
    if geo:
        g = _abi.InvrGeoOut(level, o['depth_map'].data_ptr(), o['surf_index'].data_ptr(), o['surf_depth'].data_ptr())
        _abi.check(L.invr_render_fwd_geo(*args, _abi.ptr(None, torch.int64), 0, C.byref(g)))
    else:
        _abi.check(L.invr_render_fwd(*args))
    sync()
    net._ws = None
    o['n'], o['near'], o['far'] = n, near, far
    return o


def frame_level(occ):
    """the level of the frame's crossings: the median of its non-zero occupancies (the small random-weight fields stay near 0.5, and
    a level in the middle of them gives rays that cross and rays that do not)"""
    nz = occ[occ > 0]
    assert nz.numel() > 100
    return float(nz.median())


MERGED = [(128, {}), (64, {}), (64, {'aggr': 'mean'}), (64, {'random_bg': True}), (32, {}), (24, {})]


def body_merged(S, kw, res, max_active=0):
    net = net_of(S, **kw)
    plain = abi_render(net, S, res, geo=False, max_active=max_active)
    if max_active:
        assert int(plain['stats'][6]) != 0, 'max_active is below the survivor count'
    level = frame_level(plain['raw'][:, 3])
    geo = abi_render(net, S, res, geo=True, max_active=max_active, level=level)
    for k in ('rgb_map', 'acc_map', 'raw'):
        assert same_bits(geo[k], plain[k]), k
    assert torch.equal(geo['stats'], plain['stats'])
    assert same_bits(geo['occ'].reshape(-1), plain['raw'][:, 3])
    n = geo['n']
    for k in ('depth_map', 'surf_index', 'surf_depth'):
        assert (bits(geo[k][n:]) == MARK).all(), k
    eps = 1.0 if kw.get('random_bg') else 0.0
    dm, si, sd = depth_fwd(geo['occ'].cpu().numpy(), geo['near'].cpu().numpy(), geo['far'].cpu().numpy(), None, eps, level=level)
    assert same_bits(geo['depth_map'][:n].cpu(), dm), 'depth_map'
    assert torch.equal(geo['surf_index'][:n].cpu(), si), 'surf_index'
    assert same_bits(geo['surf_depth'][:n].cpu(), sd), 'surf_depth'
    hit = si >= 0
    print('S %d %s: %d rays, %d cross %.3f, depth in [%.3f, %.3f]' % (S, kw, n, int(hit.sum()), level, float(dm.min()), float(dm.max())))
    assert 0 < int(hit.sum()) < n and float(dm.max()) > 0
    return geo


@pytest.mark.parametrize('S,kw', MERGED)
def test_depth_pass_behind_a_render_equals_the_dense_form(S, kw):
    body_merged(S, kw, RES)


def test_depth_pass_with_overflowed_survivors_reads_zeros():
    net = net_of(64)
    full = abi_render(net, 64, RES, geo=False)
    body_merged(64, {}, RES, max_active=int(full['stats'][0]) // 2)


# ---- 3. stencil -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 5, 70])
def test_stencil_points_and_directions(n):
    L = _abi.lib()
    g = np.random.RandomState(n)
    nr, h = 2 * n + 3, 0.005
    o = g.uniform(-2, 2, (nr, 3)).astype(np.float32)
    d = g.normal(size=(nr, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    z = g.uniform(0.5, 4.0, nr).astype(np.float32)
    rows = np.sort(g.choice(nr, n, replace=False)).astype(np.int32)
    o_d, d_d, z_d, rows_d = [torch.from_numpy(a).to(DEV) for a in (o, d, z, rows)]          # (held until the kernel has run)
    pts = prefilled((6 * n + 2) * 3, 6 * n * 3).view(-1, 3)
    dirs = prefilled((6 * n + 2) * 3, 6 * n * 3).view(-1, 3)
    _abi.check(L.invr_surface_stencil(_abi.ptr(o_d), _abi.ptr(d_d), _abi.ptr(z_d), _abi.ptr(rows_d, torch.int32), n, h, _abi.ptr(pts), _abi.ptr(dirs),
                                      _abi.stream_ptr()))
    sync()
    pts, dirs = pts.cpu(), dirs.cpu()
    assert (bits(pts[6 * n:]) == MARK).all() and (bits(dirs[6 * n:]) == MARK).all(), 'rows outside the list are untouched'
    want, x = R.stencil64(o, d, z, rows, h)
    o6, zd6, x6 = [np.repeat(a, 6, axis=0) for a in (np.abs(o[rows].astype(np.float64)), np.abs(z[rows, None].astype(np.float64) * d[rows]), np.abs(x))]
    bound = U * (2 * (o6 + zd6) + x6 + h)
    err = np.abs(pts[:6 * n].numpy().astype(np.float64) - want)
    print('stencil n = %d: max error / bound = %.3f' % (n, float((err / bound).max())))
    assert (err <= bound).all()
    assert np.array_equal(dirs[:6 * n].numpy().view(np.int32), np.repeat(d[rows], 6, axis=0).view(np.int32))
    # the six points of a ray differ from each other in the moved coordinate only
    p = pts[:6 * n].numpy().reshape(n, 6, 3)
    for k in range(6):
        other = [c for c in range(3) if c != k // 2]
        assert np.array_equal(p[:, k, other], p[:, k ^ 1, other])
        assert ((p[:, k, k // 2] > p[:, k ^ 1, k // 2]) == (k % 2 == 0)).all()


# ---- 4. normals on synthetic sextuples -------------------------------------------------------------------------------------------
def normals_fwd(occ6, rows, nr):
    L = _abi.lib()
    n = occ6.shape[0]
    normal = torch.full((nr, 3), MARK, dtype=torch.int32).view(torch.float32).to(DEV)
    mask = torch.full((nr,), 0x5A, dtype=torch.uint8, device=DEV)
    occ6_d, rows_d = torch.from_numpy(occ6).to(DEV), torch.from_numpy(rows).to(DEV)          # (held until the kernel has run)
    _abi.check(L.invr_stencil_normals(_abi.ptr(occ6_d), _abi.ptr(rows_d, torch.int32), n,
                                      _abi.ptr(normal), _abi.ptr(mask, torch.uint8), _abi.stream_ptr()))
    sync()
    return normal.cpu(), mask.cpu()


def check_normals(occ6, rows, normal, mask, nr):
    want, ok = R.normals64(occ6)
    listed = np.zeros(nr, bool)
    listed[rows] = True
    assert (bits(normal)[torch.from_numpy(~listed)] == MARK).all() and (mask[torch.from_numpy(~listed)] == 0x5A).all(), 'a row outside the list was written'
    got = normal.numpy()[rows].astype(np.float64)              # every listed row is compared
    assert np.array_equal(mask.numpy()[rows], ok.astype(np.uint8))
    assert (np.abs(got - want) <= 6 * U).all(), float(np.abs(got - want).max())
    assert (np.abs(np.linalg.norm(got[ok], axis=1) - 1.0) <= 4 * U).all()
    assert (bits(normal)[torch.from_numpy(rows[~ok].astype(np.int64))] == 0).all(), 'a degenerate row is three +0'
    return ok


@pytest.mark.parametrize('n', [1, 7, 300])
def test_normals_on_synthetic_sextuples(n):
    g = np.random.RandomState(10 + n)
    nr = 2 * n + 5
    occ6 = g.uniform(0.0, 1.0, (n, 6)).astype(np.float32)
    if n >= 7:
        occ6[1] = 0.3                                             # zero gradient
        occ6[2, [1, 3, 5]] = occ6[2, [0, 2, 4]]                   # zero gradient, pairwise
        occ6[3, 0] = np.inf                                       # an infinity
        occ6[4, :2] = np.inf                                      # inf - inf
        occ6[5, 2] = np.nan
    rows = np.sort(g.choice(nr, n, replace=False)).astype(np.int32)
    normal, mask = normals_fwd(occ6, rows, nr)
    ok = check_normals(occ6, rows, normal, mask, nr)
    assert ok.sum() == (n - 5 if n >= 7 else n)


# ---- 5. geomaps.geometry_maps on the small scene ---------------------------------------------------------------------------------
def test_geometry_maps_of_the_small_scene():
    from invr import geomaps
    S = 64
    net = net_of(S)
    b, (ro, rd, near, far) = frame(RES)
    n = ro.shape[0]
    # the random-weight field of make_scene's own frame stays close to 0.5 and need not cross it: the level is the median of the frame's
    # non-zero occupancies (the issue's fallback; the golden frame's 370 of 447 crossings at 0.5 are a property of that frame)
    level = frame_level(abi_render(net, S, RES, geo=False)['raw'][:, 3])
    h = 0.005
    maps = geomaps.geometry_maps(net, b, level=level, h=h)
    sync()
    assert set(maps) == {'depth_map', 'surf_depth', 'surf_mask', 'surf_normal', 'acc_map', 'rgb_map'}
    shapes = {'depth_map': (n,), 'surf_depth': (n,), 'surf_mask': (n,), 'surf_normal': (n, 3), 'acc_map': (n,), 'rgb_map': (n, 3)}
    for k, v in maps.items():
        assert tuple(v.shape) == shapes[k] and v.dtype == (torch.bool if k == 'surf_mask' else torch.float32) and v.device == ro.device, k
    m = maps['surf_mask']
    assert 0 < int(m.sum()) < n
    # the same maps as the ABI render; the normal recomputed from the field at the stencil rebuilt here
    geo = abi_render(net, S, RES, geo=True, level=level)
    assert same_bits(maps['depth_map'], geo['depth_map'][:n]) and same_bits(maps['surf_depth'], geo['surf_depth'][:n])
    assert same_bits(maps['rgb_map'], geo['rgb_map']) and same_bits(maps['acc_map'], geo['acc_map'])
    rows = torch.nonzero(geo['surf_index'][:n] >= 0).reshape(-1)
    # fmaf(z, d, o): the product of two fp32 is exact in float64 and the sum is rounded to fp32 from there; then one fp32 addition of h
    x = (geo['surf_depth'][:n][rows, None].cpu().numpy().astype(np.float64) * rd[rows].cpu().numpy().astype(np.float64)
         + ro[rows].cpu().numpy().astype(np.float64)).astype(np.float32)
    pts = np.repeat(x[:, None, :], 6, axis=1)
    for k in range(6):
        pts[:, k, k // 2] = x[:, k // 2] + np.float32(-h if k % 2 else h)
    pts = torch.from_numpy(pts.reshape(-1, 3)).to(DEV)
    with torch.no_grad():
        occ6 = net.forward(pts, rd[rows].repeat_interleave(6, 0), None, b)['occ'].reshape(-1, 6)
    sync()
    want, ok = R.normals64(occ6.cpu().numpy())
    rows = rows.cpu()
    assert torch.equal(m.cpu()[rows], torch.from_numpy(ok)) and int(m.sum()) == int(ok.sum())
    got = maps['surf_normal'].cpu()
    err = np.abs(got[rows].numpy().astype(np.float64) - want)
    print('geometry_maps: %d of %d rays cross %.3f, %d normals, max error %.2f u' % (len(rows), n, level, int(ok.sum()), float(err.max()) / U))
    assert (err <= 6 * U).all()
    assert (np.abs(np.linalg.norm(got[rows].numpy().astype(np.float64)[ok], axis=1) - 1.0) <= 4 * U).all()
    rest = torch.ones(n, dtype=torch.bool)
    rest[rows] = False
    assert (bits(got)[rest] == 0).all() and not m.cpu()[rest].any()
    # image_of places every value at its pixel
    H, W = int(b['H']), int(b['W'])
    at = b['mask_at_box'][0].reshape(-1).cpu().bool()
    for k in ('depth_map', 'surf_normal', 'surf_mask'):
        img = geomaps.image_of(maps[k], b)
        assert tuple(img.shape) == (H, W) + tuple(maps[k].shape[1:]) and img.dtype == maps[k].dtype
        flat = img.reshape((H * W,) + tuple(maps[k].shape[1:])).cpu()
        assert torch.equal(flat[at], maps[k].cpu()) and not flat[~at].any()
    # normals=False: the rays that cross
    quick = geomaps.geometry_maps(net, b, level=level, normals=False)
    assert torch.equal(quick['surf_mask'].cpu(), (geo['surf_index'][:n] >= 0).cpu()) and not quick['surf_normal'].any()


def test_run_geometry_loops_over_a_sequence():
    from invr import driver
    net = net_of(64)
    b, _ = frame(RES)
    seen = []
    assert driver.run_geometry(net, [b, b], on_frame=lambda i, m: seen.append((i, m)), level=0.5, normals=False, device=DEV) is None
    assert [i for i, _ in seen] == [0, 1] and same_bits(seen[0][1]['depth_map'], seen[1][1]['depth_map'])
    out = driver.run_geometry(net, [b], level=0.5, normals=False, device=DEV)
    assert len(out) == 1 and same_bits(out[0]['depth_map'], seen[0][1]['depth_map'])


# ---- 6. Renderer.render with cfg.render_depth ------------------------------------------------------------------------------------
def test_renderer_carries_the_depth_maps_in_all_three_eval_paths(monkeypatch):
    from invr import renderer as RD
    S = 64
    b, (ro, _, _, _) = frame(RES)
    n = ro.shape[0]
    base = net_of(S)
    level = frame_level(abi_render(base, S, RES, geo=False)['raw'][:, 3])
    net = net_of(S, render_depth=True, surface_level=level)
    want = abi_render(net, S, RES, geo=True, level=level)

    def check(ret, host):
        assert set(ret.keys()) == {'rgb_map', 'acc_map', 'depth_map', 'surf_depth', 'raw', 'occ'}
        for k in ('depth_map', 'surf_depth'):
            assert tuple(ret[k].shape) == (1, n) and ret[k].is_cuda != host, k
            assert same_bits(ret[k][0].cpu(), want[k][:n].cpu()), k
        assert same_bits(ret['rgb_map'][0].cpu(), want['rgb_map'].cpu())

    for to_cpu in (True, False):
        r = RD.Renderer(net)
        r.eval_to_cpu = to_cpu
        check(r.render(b), to_cpu)                                   # the synchronous path
        with monkeypatch.context() as mp:                            # the chunked path: 7 calls
            mp.setattr(RD, 'MAX_SAMPLES_PER_CALL', (n // 7 + 1) * S)
            check(r.render(b), to_cpu)
        if DEV != 'cpu':
            r2 = RD.Renderer(net)
            r2.eval_to_cpu, r2.in_flight = to_cpu, 2                 # frames in flight
            rets = [r2.render(b) for _ in range(3)]
            assert all('depth_map' in x and 'surf_depth' in x for x in rets)
            for x in rets:
                check(x, to_cpu)
            r2.flush(release=True)
    # the flag off: exactly today's keys
    off = RD.Renderer(base)
    assert set(off.render(b).keys()) == {'rgb_map', 'acc_map', 'raw', 'occ'}
