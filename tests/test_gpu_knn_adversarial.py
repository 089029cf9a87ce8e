"""GPU: the 4-nearest-neighbour kernels (csrc/k_knn.hip) on the degenerate vertex sets of tests/knn_cases.py.

A. The brute-force stage kernel (k_knn_dense through invr_knn_neighbors / invr_knn_blend) — the yardstick of everything below —
   against the EXACT integer reference on dyadic vertices and queries: rows and squared distances with no tolerance, weights /
   distance / blend weights against float64 on those exact distances.
B. The production pair kernel (k_knn_pairs + k_pair_lists, through Network.geometry_pass and Network.render_rays) against that
   brute-force kernel on the identical pose points, bit for bit, for every survivor and all five parts (the checker of
   tests/test_gpu_production_kernels.py), on every scene of tests/knn_cases.py: parts of 64 and of more than 64 clusters, the LDS
   carve boundary and the device-side fallback behind it, parts of 3 .. 17 vertices, exact distance ties, coplanar / collinear /
   single-point parts, pose space 8 m from the origin, coarse and partly missed lattices; ray frames of 2 - 64 samples and point frames
   (Network.forward: ONE sample per point) on both sides of the front plan's N >= 4 cells switch.
C. One workspace reused across frames of different scenes.

tests/test_hostsim_knn_cpu.py runs the same bodies on the CPU wave machine with the reduced size table."""
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_production_kernels as P          # noqa: E402  (check_pairs)
from tests import knn_cases as K                      # noqa: E402
from invr import _abi, scene, stages                  # noqa: E402

DEV = 'cuda:0'
U = 2.0 ** -24

# ---- sizes (tests/test_hostsim_knn_cpu.py swaps in a reduced table) --------------------------------------------------------------
# A run = one frame: rays x S samples at smpl_thresh `thresh`; all_survive = distance channel 0 (every ray-sample inside the lattice
# survives the cull, Na = rays * S); side = which side of the front plan's N >= 4 * cells switch the run must be on ('ge': masked
# cull with the lattice classes in the same launch — fast / ray4 / dilated mask when S % 4 == 0 and no jitter; 'lt': unmasked cull
# and a stand-alone k_knn_voxel_class), asserted from the batch.
RUNS = {
    'full64': dict(rays=4096, S=64, thresh=0.05, side='ge'),
    's16': dict(rays=4096, S=16, thresh=0.05, side='lt'),
    'jit30': dict(rays=2048, S=30, thresh=0.1, all_survive=True, jitter=True, side='lt'),
    # jittered AND masked (not fast): edges_b, where 4096 x 30 samples reach 4 per cell
    'jit30ge': dict(rays=4096, S=30, thresh=0.05, jitter=True, side='ge'),
    'two': dict(rays=1024, S=2, thresh=0.1, all_survive=True, side='lt'),      # (the smallest RAY frame: geometry_pass / render_rays refuse S = 1)
    # S = 1: Network.forward on world points (invr_field_fwd: the wpts arm of the front plan — never fast, masked from 4 points per cell)
    'pts_ge': dict(rays=262144, S=1, thresh=0.05, mode='points', side='ge'),
    'pts_lt': dict(rays=16384, S=1, thresh=0.1, all_survive=True, mode='points', side='lt'),
    # edges_c only: the "provably unflagged" class disabled (near_hi2 = +inf, band_lo2 = 0 in make_scene_dev), and a threshold at
    # which it takes nearly every pair
    'class_off': dict(rays=2048, S=16, thresh=0.45),
    'tiny': dict(rays=2048, S=16, thresh=1e-3, all_survive=True),
    # the whole eval pipeline (depth-windowed survivor order: S a power of two, no jitter)
    # (without z_vals / weights outputs and with S % 4 == 0 this is the front plan's ray4 + dilated-mask arm)
    'render64': dict(rays=4096, S=64, thresh=0.05, mode='render', side='ge'),
    # masked and fast, but S % 4 != 0: not ray4 (edges_b and the coarse lattices: the scenes where 4096 x 30 samples reach 4 per cell)
    's30': dict(rays=4096, S=30, thresh=0.05, side='ge'),
}
# the coarse lattices have 665 cells (every run but `two` is on the 'ge' side) and interpolate the distance over 0.1 m cells: next
# to nothing survives at 0.05
OVERRIDE = {('coarse', 'full64'): dict(thresh=0.1), ('coarse_tight', 'full64'): dict(thresh=0.1),
            ('coarse', 's16'): dict(thresh=0.1, side='ge'), ('coarse_tight', 's16'): dict(thresh=0.1, side='ge'),
            ('coarse', 's30'): dict(thresh=0.1), ('coarse_tight', 's30'): dict(thresh=0.1),
            ('coarse', 'jit30'): dict(side='ge'), ('coarse_tight', 'jit30'): dict(side='ge'),
            ('coarse', 'pts_ge'): dict(thresh=0.1), ('coarse_tight', 'pts_ge'): dict(thresh=0.1),
            ('coarse', 'pts_lt'): dict(rays=2048), ('coarse_tight', 'pts_lt'): dict(rays=2048)}
MINC = 200                     # least count of listed / far / unflagged-beside-near pairs (and of 4th/5th ties) per run
# documented exceptions: counts a scene's geometry or a run's threshold cannot reach (never all of a run's counts)
#   class_off: dist = d w / (w + 1e-8) never reaches 0.45 m (its maximum over d is ~0.44 m): every pair inside the fold distance is flagged
#   dup2 / dup4 with generic float positions: every vertex has the SAME multiplicity 2 (4), so the 4th and 5th nearest distances
#   differ (the list ends on a multiplicity boundary); their ties sit INSIDE the list — counted instead (`tie_in`).  The dyadic
#   variants collide further on the lattice (multiplicities 2, 4, 6, ..): ties on the 4th/5th boundary.
EXEMPT = {'class_off': ('unflagged',)}
TIE_45 = ('dup2-block-dyadic', 'dup4-interleaved-dyadic', 'lattice')
TIE_IN = ('dup2-interleaved', 'dup4-block')
A_N = (1, 255, 256, 257, 1000)
A_TIES = 1000
ASSERT_SIDES = True

PAIR_CASES = [(s, r) for s in K.SCENES for r in ('full64', 's16', 'jit30', 'two', 'pts_ge', 'pts_lt')] + \
             [('edges_c', 'class_off'), ('edges_c', 'tiny'), ('edges_b', 'jit30ge'), ('edges_b', 's30'), ('coarse', 's30'), ('coarse_tight', 's30')] + \
             [(s, 'render64') for s in ('dup2-interleaved', 'edges_c', 'carve_spill')]


def ids(cases):
    return ['-'.join(str(x) for x in c) for c in cases]


@functools.lru_cache(maxsize=4)
def scene_batch(name, all_survive):
    return K.build(name, all_survive=all_survive)


@pytest.fixture(scope='module')
def small_net():
    from invr.config import make_cfg
    from invr.network import Network
    torch.manual_seed(11)
    cfg = make_cfg(table_log2=12)
    net = Network(cfg=copy.deepcopy(cfg)).to(DEV).eval()
    return cfg, net


# ---- A: brute force against the exact reference ----------------------------------------------------------------------------------
# vertex sets / query blocks (units of 2^-5 m): every 4th-nearest distance^2 of a part with >= 4 vertices stays below 0.95 m^2
# (x > -85: exp(x) a normal fp32 number — a relative allowance means nothing on a denormal), asserted from the reference
A_SCENES = {
    'lattice': (lambda: K.lattice(), ((-6, 0, -4), (6, 14, 4))),                              # lengths 2047, 2049, 2048, 200, 70
    'lattice-4097': (lambda: K.lattice(lengths=(4097, 3, 2048, 64, 70)), ((-6, 0, -4), (6, 14, 4))),
    'dup4-dyadic': (lambda: K.build('dup4-interleaved-dyadic'), ((-6, -10, -4), (6, 4, 4))),
}
# allowance = C_A * |fp32 torch evaluation - float64| + (K_A + 2 |x|) 2^-24 |value|   (tests/conditioning.py's convention)
C_A, K_A = 4.0, 4.0


@functools.lru_cache(maxsize=None)
def a_case(tag):
    build, (lo, hi) = A_SCENES[tag]
    b = build()
    q = K.query_block(lo, hi, n=max(A_N))
    L = b['lengths2'][0]
    assert b['part_pts'].shape[2] > int(L.max())                               # part_stride M > len
    rows, d2 = K.exact_knn(q, b['part_pts'][0], L, 5)
    w, dist, bw, x = K.blend_reference(d2[..., :4], rows[..., :4], b['part_pbw'][0])
    full = L >= 4
    assert float(d2[:, full, 3].max()) < 0.95
    ties = int(((d2[..., 3] == d2[..., 4]) & np.isfinite(d2[..., 4]))[:, full].sum())
    return dict(b=b, q=q, L=L, rows=rows, d2=d2, w=w, dist=dist, bw=bw, x=x, full=full, ties=ties)


def device_scene(b, thresh=0.05):
    from invr.config import make_cfg
    gb = {k: v.to(DEV) for k, v in scene.to_torch(b).items()}
    cfg = make_cfg(table_log2=12)
    cfg.smpl_thresh = thresh
    keep = [gb]
    return _abi.make_scene(gb, cfg, keep), keep


def blend32(d2, rows, pbw):
    """the kernel's operations (knn_weights + the 24-joint blend of k_knn_dense), one fp32 torch op each, on the exact distances"""
    d = d2.sqrt()
    e = torch.exp(-(d * d) / K.TWO_R2)
    den = (((e[..., 0] + e[..., 1]) + e[..., 2]) + e[..., 3]) + K.KNN_EPS
    w = e / den[..., None]
    dist = torch.zeros_like(den)
    bw = torch.zeros(d2.shape[:2] + (24,), dtype=d2.dtype, device=d2.device)
    for k in range(4):
        dist = dist + d[..., k] * w[..., k]
        for p in range(d2.shape[1]):
            bw[:, p] = bw[:, p] + pbw[p][rows[:, p, k]] * w[:, p, k, None]
    return w, dist, bw


def run_dense_case(tag, n):
    """invr_knn_neighbors / invr_knn_blend on n dyadic queries: rows and squared distances EQUAL the integer reference (ties by row,
    only the first lengths2[p] rows: the rows behind hold decoys), a part with fewer than 4 vertices ends in (+inf, row 0) entries and
    a NaN distance; w / dist / bw within  C_A |fp32 torch - float64| + (K_A + 2 |x|) 2^-24 |value|  of float64 on the exact distances,
    x = -d^2 / 0.01125 of the element (w) or of the 4th neighbour (dist, bw: the worst-conditioned term stands for the whole sum — an
    UPPER bound of the sum's conditioning, up to ~170 units of 2^-24 at x = -85).
    Measured worst err / (|fp32 torch - float64| + (1 + 2 |x|) 2^-24 |value|), i.e. the constants the kernel needs when C = K:
    0.950 on MI355X (n = 1000: lattice 0.940, lattice-4097 0.949, dup4-dyadic 0.950; 0.54 .. 0.77 for the smaller n), 0.70 on the CPU
    wave machine; C_A = K_A = 4 is that with x4 headroom."""
    c = a_case(tag)
    L, full = c['L'], c['full']
    sc, keep = device_scene(c['b'])
    q = torch.from_numpy(c['q'][:n]).to(DEV)
    nn, d2, w, dist = stages.knn_neighbors(sc, q)
    bw, dist_b = stages.knn_blend(sc, q)
    nn, d2, w, dist, bw, dist_b = (t.cpu().numpy() for t in (nn, d2, w, dist, bw, dist_b))
    assert np.array_equal(dist, dist_b, equal_nan=True)
    for p in range(5):
        kk = min(4, int(L[p]))
        assert np.array_equal(nn[:, p, :kk], c['rows'][:n, p, :kk]), (tag, n, p)
        assert np.array_equal(d2[:, p, :kk].astype(np.float64), c['d2'][:n, p, :kk]), (tag, n, p)
        if kk < 4:
            assert np.isposinf(d2[:, p, kk:]).all() and (nn[:, p, kk:] == 0).all() and np.isnan(dist[:, p]).all()
    # weights, distance, blend weights of the parts with >= 4 vertices
    d2_t = torch.from_numpy(c['d2'][:n, :, :4].astype(np.float32)).to(DEV)
    rows_t = torch.from_numpy(c['rows'][:n, :, :4]).to(DEV)
    pbw_t = torch.from_numpy(c['b']['part_pbw'][0]).to(DEV)
    w32, dist32, bw32 = (t.cpu().numpy().astype(np.float64) for t in blend32(d2_t, rows_t, pbw_t))
    ax = np.abs(c['x'][:n])
    worst = 0.0
    for name, got, t32, ref, cond in (('w', w, w32, c['w'][:n], ax), ('dist', dist, dist32, c['dist'][:n], ax[..., 3]),
                                      ('bw', bw, bw32, c['bw'][:n], ax[..., 3:4])):
        got, t32, ref, cond = got[:, full], t32[:, full], ref[:, full], np.broadcast_to(cond, ref.shape)[:, full]
        err, dev = np.abs(got - ref), np.abs(t32 - ref)
        unit = dev + (1.0 + 2.0 * cond) * U * np.abs(ref)
        ratio = float(np.max(np.where(err > 0, err / np.maximum(unit, 1e-300), 0.0)))
        worst = max(worst, ratio)
        tol = C_A * dev + (K_A + 2.0 * cond) * U * np.abs(ref)
        assert bool((err <= tol).all()), (tag, n, name, ratio, float(err.max()))
    print('knn dense %s n=%d: worst err / (|fp32 torch - f64| + (1 + 2|x|) u |value|) = %.3f' % (tag, n, worst))
    return worst


@pytest.mark.parametrize('tag,n', [(t, n) for t in A_SCENES for n in A_N], ids=ids([(t, n) for t in A_SCENES for n in A_N]))
def test_dense_knn_vs_exact_reference(tag, n):
    run_dense_case(tag, n)


def test_exact_reference_has_ties_on_the_list_boundary():
    """At least 1000 of the (point, part) pairs test A checks have d^2[3] == d^2[4] bit-exactly — the 4th and the 5th nearest vertex
    tie, the row half of the key alone decides which one is listed — counted from the integer reference alone (n = 1000: lattice 3985,
    lattice-4097 2378, dup4-dyadic 1433 of 5000 / 4000 / 5000 pairs; printed)."""
    per = {t: a_case(t)['ties'] for t in A_SCENES}
    print('4th/5th ties in the reference:', per)
    assert sum(per.values()) >= A_TIES and min(per.values()) > 0, per


# ---- B: the pair kernel against brute force --------------------------------------------------------------------------------------
def run_frame(net_cfg, name, run, fresh=True):
    """One frame of scene `name` under the run `run` (RUNS) through geometry_pass / render_rays, and views of what it left behind"""
    cfg0, net = net_cfg
    r = dict(RUNS[run])
    r.update(OVERRIDE.get((name, run), {}))
    S, n = r['S'], r['rays']
    points = r.get('mode') == 'points'
    b = scene_batch(name, bool(r.get('all_survive')))
    if points:
        wp, wd = K.world_points(b, n, seed=len(run))
        # the same points as a ray list for stages.pose_points, which wants two samples per ray: o + 0 * z = o exactly, so sample 0 of
        # "ray" i is point i through the very sample_pose_point code
        b = dict(b, ray_o=wp[None], ray_d=np.zeros_like(wp)[None], near=np.zeros(n, np.float32)[None], far=np.ones(n, np.float32)[None])
        for k in ('rgb', 'occupancy', 'mask_at_box'):
            b.pop(k, None)
    else:
        b = K.rays(b, n, seed=len(run), inner=(S == 2))
    if ASSERT_SIDES and r.get('side'):
        assert (n * S >= 4 * K.cells(b)) == (r['side'] == 'ge'), (name, run, n * S, K.cells(b))
    gb = {k: v.to(DEV) for k, v in scene.to_torch(b).items()}
    cfg = copy.deepcopy(cfg0)
    cfg.smpl_thresh = r['thresh']
    jit = None
    if r.get('jitter'):
        jit = torch.rand(n, S, generator=torch.Generator().manual_seed(3)).to(DEV)
    old = net.cfg
    net.cfg = cfg
    try:
        ctx = net.prepare(gb)
        ro, rd, nr, fa = (gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far'))
        if fresh:
            net._ws = None
        if points:
            assert S == 1
            field = net.forward(ro, torch.from_numpy(wd).to(DEV), None, ctx)
            assert field['raw'].shape == (1, n, 4) and bool(torch.isfinite(field['raw']).all())
            out = {'_ws': (net._ws, n, 1, 0)}
        elif r.get('mode') == 'render':
            out = net.render_rays(ctx, ro, rd, nr, fa, S, want_raw=False)
        else:
            out = net.geometry_pass(ctx, ro, rd, nr, fa, S, jitter=jit)
        torch.cuda.synchronize()
        if fresh:
            net._ws = None
    finally:
        net.cfg = old
    v = _abi.ws_views(*out['_ws'])
    st = (v['counters'] if points else out['stats']).cpu().numpy()[:16]       # (stats = the first CNT_LEN counters; forward returns none)
    assert st[6] == 0
    Na = int(st[0])
    act = v['active_idx'][:Na]
    if points:
        pts, dirs = stages.pose_points(ctx.scene, ro, rd, nr, fa, 2, 2 * act)
    else:
        pts, dirs = stages.pose_points(ctx.scene, ro, rd, nr, fa, S, act, jitter=jit)
    return dict(k='%s-%s' % (name, run), name=name, run=run, cfg=cfg, net=net, b=b, gb=gb, ctx=ctx, out=out, st=st, v=v, Na=Na, act=act,
                pts=pts, dirs=dirs, thresh=r['thresh'], S=S, dev=DEV, jit=jit, points=points)


def check_survivors(f):
    """the survivor set = what the dense stage path keeps (stages.pose_points + sample_volume + `< thresh`), every ray-sample"""
    from invr.autograd import sample_volume
    gb, S = f['gb'], f['S']
    ro, rd, nr, fa = (gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far'))
    vol, bounds = gb['pbw'][0].contiguous(), gb['pbounds'][0].contiguous()
    if f['points']:
        pts = stages.pose_points(f['ctx'].scene, ro, rd, nr, fa, 2, want_dirs=False)[0][0::2]
    else:
        pts, _ = stages.pose_points(f['ctx'].scene, ro, rd, nr, fa, S, jitter=f['jit'], want_dirs=False)
    pn = sample_volume(vol, bounds, pts, vol.shape[3] - 1, 1)[:, 0]
    want = (pn < f['thresh']).nonzero(as_tuple=True)[0]
    got = f['act'].long().sort()[0]
    assert want.numel() == f['Na'] and torch.equal(got, want), (f['k'], want.numel(), f['Na'])


def check_frame(f, minc=None):
    """check_survivors + the pair checker + the run's non-vacuity counts, the latter from the brute-force results only"""
    minc = MINC if minc is None else minc
    check_survivors(f)
    # the far-fold distance the frame derived (part_prepare_body) against the rule restated from the batch's matrices; the checker
    # then holds the far pairs to the RESTATED value
    want_dfar2 = K.far_dist2(f['b'])
    got_dfar2 = float(f['v']['knn_dfar2'][0])
    if want_dfar2 == 0.4624:
        assert got_dfar2 == float(np.float32(0.4624)), got_dfar2
    else:                                                                      # (logf in fp32 on the device)
        assert np.isfinite(got_dfar2) and abs(got_dfar2 - want_dfar2) <= 1e-5 * want_dfar2, (got_dfar2, want_dfar2)
    dfar2 = float(np.float32(want_dfar2)) * ((1.0 - 1e-5) if want_dfar2 > 0.4624 else 1.0)
    nn, d2, w, dist = P.check_pairs(f, dict(na=minc, listed=-1), dfar2=dfar2)
    name, run, thresh = f['name'], f['run'], f['thresh']
    L = f['b']['lengths2'][0]
    ok = torch.from_numpy(L >= 4).to(dist.device)
    flag = dist < thresh                                                       # (NaN: a part with fewer than 4 vertices, never flagged)
    assert not bool(flag[:, ~ok].any())
    beyond = d2[:, :, 0] > dfar2
    listed = flag & ~beyond
    cnt = dict(listed=int(listed.sum()), far=int((flag & beyond).sum()),
               unflagged=int((~flag & ~beyond & ok[None]).any(1).sum()))       # survivors with an unflagged pair that is not far
    nn_np, listed_np = nn.cpu().numpy(), listed.cpu().numpy()
    if name in TIE_45:
        cnt['tie45'] = int((K.tie_45(nn_np, f['b']['part_pts'][0], L) & listed_np).sum())
    if name in TIE_IN:
        cnt['tie_in'] = int(((d2[:, :, 0] == d2[:, :, 1]) & listed).sum())
    print('knn pairs %s: Na %d, per part %s, %s' % (f['k'], f['Na'], [int(x) - 1 for x in f['st'][1:6]], cnt))
    for key, c in cnt.items():
        if key in EXEMPT.get(run, ()):
            continue
        assert c >= minc, (f['k'], key, c)
    return cnt


@pytest.mark.parametrize('name,run', PAIR_CASES, ids=ids(PAIR_CASES))
def test_knn_pairs_vs_brute_force(small_net, name, run):
    """k_knn_pairs on a degenerate scene: survivor set and slot map, listed | far == (dist < thresh), far => d2[0] > dfar2, lists
    ascending and complete, counters, l_nn EQUAL to invr_knn_neighbors (a placeholder that survived the sweep would show as a row of
    another vertex), l_w within 1 ulp — for every survivor and part.  Counts per run (>= 200 each; printed): listed pairs, pairs
    beyond the far-fold distance, survivors with an unflagged pair inside it; 4th/5th ties for the dyadic dup scenes and `lattice`,
    ties inside the list for the float dup scenes.  Measured on the `full64` run (survivors: listed / beyond / unflagged / ties):
      dup2-interleaved 18436: 33421 / 21938 / 14989 / 33421 in the list      dup2-block-dyadic 19756: 35259 / 23480 / 16131 / 14700 4th-5th
      dup4-block 17621: 31546 / 21058 / 14346 / 31546 in the list            dup4-interleaved-dyadic 18482: 32834 / 21967 / 15033 / 7362 4th-5th
      lattice 26489: 46176 / 42848 / 24656 / 15278 4th-5th                    edges_a 6354: 8940 / 16759 / 5633
      edges_b 11923: 15182 / 22459 / 9313 (part 0, 3 vertices: 0 pairs)       edges_c 8117: 13987 / 14660 / 7212
      carve_fit 18199: 37485 / 15072 / 14298 (38724 listed by the LDS sweep)  carve_spill 11284: 23471 / 10411 / 8621 (23471 by the fallback)
      offset 8117: 13987 / 14660 / 7212                                       coarse 27870: 55889 / 32355 / 22138
      coarse_tight 60144: 120394 / 70418 / 48474
    The smallest counts of any run are those of the 2048-sample `two` frames: listed 1563, beyond 3495, unflagged 1324, 4th/5th ties 478
    (lattice), ties in the list 2416; edges_c at 0.45: 57941 / 45139 / 0 (the documented exception), at 1e-3: 22423 / 87635 / 25371.
    Point frames (S = 1): 262144 points leave 6954 (edges_a) .. 60300 (coarse_tight) survivors with counts like full64's; the smallest,
    2048 points on the coarse lattices: 2401 / 3605 / 1620.  edges_b jittered and masked: 4970 survivors, 6322 / 9299 / 3932."""
    if name in ('carve_fit', 'carve_spill'):
        slots = K.padded_slots(scene_batch(name, False)['lengths2'][0])
        assert (slots > K.LDS_SLOTS) == (name == 'carve_spill') and slots in (7680, 7744)
    f = run_frame(small_net, name, run)
    cnt = check_frame(f)
    if name in ('carve_fit', 'carve_spill'):
        # which path ran: the brute-force fallback folds EVERY pair beyond the far distance (exact nearest distance), the LDS-resident
        # sweep only those its cluster bounds prove far — it lists the remaining band pairs
        n_listed = sum(int(x) - 1 for x in f['st'][1:6])
        assert n_listed == cnt['listed'] if name == 'carve_spill' else n_listed > cnt['listed'], (name, n_listed, cnt)


# ---- C: one workspace, four frames -----------------------------------------------------------------------------------------------
REUSE = [('edges_c', 'full64'), ('coarse', 's16'), ('lattice', 'jit30'), ('dup4-block', 'full64'), ('edges_c', 'full64')]


def test_workspace_reused_across_scenes(small_net):
    """edges_c, coarse, lattice, dup4, edges_c again through ONE buffer (asserted: the same address in every frame; the production
    tests drop it around every frame): the lattice classes, ticket counters and group counts of another scene's frame are in it when
    the next frame starts.  The dup4 frame has the (rays, S) of the edges_c frames, so every array of the last frame starts out holding
    ANOTHER scene's frame of the same layout; the two smaller frames in between leave a mixture.  Every frame passes the pair checker;
    the last leaves what the first left, bit for bit."""
    cfg0, net = small_net
    net._ws = None
    snaps, ptrs = [], []
    try:
        for name, run in REUSE:
            f = run_frame(small_net, name, run, fresh=False)
            check_frame(f)
            ptrs.append(f['out']['_ws'][0].data_ptr())
            v, Na = f['v'], f['Na']
            snap = dict(st=f['st'].copy(), act=f['act'].clone(), pf=v['pflags'][:Na].clone(), ff=v['farflags'][:Na].clone())
            for p in range(5):
                c = int(f['st'][1 + p])
                slots = v['l_slot'][p][:c - 1].long()
                snap['slot%d' % p] = v['l_slot'][p][:c].clone()
                snap['nn%d' % p], snap['w%d' % p] = v['l_nn'][p][slots].clone(), v['l_w'][p][slots].clone()
            snaps.append(snap)
    finally:
        net._ws = None
    assert len(set(ptrs)) == 1, ptrs
    a, b = snaps[0], snaps[-1]
    assert a['st'][0] >= MINC
    for k in a:
        assert np.array_equal(a[k], b[k]) if k == 'st' else torch.equal(a[k], b[k]), k


def test_one_sample_per_ray_is_refused(small_net):
    """A RAY frame needs two samples per ray (the linear depth step is 1 / (S - 1)): geometry_pass and render_rays report S = 1 as
    an error, nothing runs.  Frames of one sample exist as POINT frames (Network.forward -> invr_field_fwd): the pts_* runs above."""
    cfg0, net = small_net
    b = K.rays(scene_batch('edges_c', True), 64)
    gb = {k: v.to(DEV) for k, v in scene.to_torch(b).items()}
    ctx = net.prepare(gb)
    ro, rd, nr, fa = (gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far'))
    for call in (net.geometry_pass, net.render_rays):
        with pytest.raises(RuntimeError, match='n_samples >= 2'):
            call(ctx, ro, rd, nr, fa, 1)
    net._ws = None
