"""GPU: the part merge (csrc/k_lists.hip: k_winner_lists<0..3>, k_all_lists; csrc/k_mlp.hip: k_part_rgb_all<true>) and its transpose
(csrc/k_train.hip: k_merge_bwd<0|1|2> through invr_merge_bwd) in EVERY cfg.aggr mode, survivor by survivor against the float64
transcription of inb_part_network_multiassign.py:229-256 in tests/merge_reference.py.

The merge's inputs are read out of the workspace a render left (`_abi.ws_views`): the flag bytes, the pair lists, the per-pair [rgb, occ]
(recomputed by the one-kernel part MLP, invr_part_mlp_fwd, on the frame's own encoder outputs and held bit for bit to what the two
phases stored), the frame's own part_dist.  Every discrete decision is therefore exact — no exemption anywhere — and the sums are held to

    |kernel - exact|  <=  k 2^-24 A  +  c 2^-126          A = the sum on magnitudes, c = the number of summands; A == 0: exactly 0.0

with k from the arithmetic, not fitted: 'mean' k = 9 (at most five sequential fp32 adds and one division: the (c + 4) rule with
c = 5); 'dist' k = 16 (a weight carries at most 8.5 roundings — the add, the reciprocal, five squares summed, half of that through
the square root, the division —, one product and the five-term sum add the rest).  The transpose: '' / 'mindist' route bit copies;
'mean' |got - g / 5| <= 2 2^-24 |g / 5|, 'dist' <= 10 2^-24 |exact| on listed parts; exactly 0 elsewhere; the far row of part p =
the float64 sum over its n far contributors within (n + 4) 2^-24 A (the atomic adds come in any order).
Each case prints K = max |kernel - exact| / (2^-23 A) (profiles/merge_modes_headroom.md keeps them).

Frames (pose 2 of tests/test_gpu_production_kernels.POSES, smpl_thresh 0.1, the reduced model of tests/test_gpu_list_groups.py):
    A  the frame of check_list_groups, 96 x 96 rays x 64 samples, trimmed until Na % 8 != 0: ~45 k survivors in more than two slot
       groups, the ragged flag-byte tail, the depth-windowed survivor order
    B  the first 256 rays of A: one group
    C  48 x 48 x 96 samples: ray-major order, S not a multiple of 64
    D  A with near = far = far + 10: no survivor — every output zero, every read guarded by Na
Outputs of invr_merge_bwd are pre-filled: NaN where it must write (the far row too: the call clears it itself), a recognisable bit
pattern where it must not (asserted bit-identical afterwards).  tests/test_hostsim_merge_modes_cpu.py runs the same bodies on the host
build of the kernels."""
import copy
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import tests.test_gpu_list_groups as G               # noqa: E402
import tests.test_gpu_production_kernels as P        # noqa: E402
from tests import merge_reference as MG              # noqa: E402  (checker only)
from invr import _abi, scene                         # noqa: E402

DEV = 'cuda:0'
NAN = float('nan')
MARK = -0x365A5A5B                                   # int32 bit pattern 0xC9A5A5A5 = -1358004.6f: what no kernel may touch
GROUP = 4096
AGGRS = list(MG.AGGRS)
AGGR_CODE = {'': 0, 'mean': 1, 'dist': 2, 'mindist': 3}             # InvrScene::aggr
K_FWD = {'mean': 9.0, 'dist': 16.0}                                  # the bounds of the module docstring, in units of 2^-24 A
K_BWD = {'mean': 2.0, 'dist': 10.0}
CENSUS_MIN = 20
A_RAYS = None            # (first, last) ray of frame A; None = the whole frame (the host-build twin cuts it down)
FRAMES = ('A', 'B', 'C', 'D')
U = 2.0 ** -24
TINY = 2.0 ** -126

_batches, _trim, _frames, HEADROOM = {}, {}, {}, {}


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def batch(res):
    if res not in _batches:
        kw = dict(P.POSES[G.POSE])
        thresh = kw.pop('thresh')
        bnp, _ = scene.make_scene(res, res, **kw)
        _batches[res] = ({k: v.to(DEV) for k, v in scene.to_torch(bnp).items()}, thresh)
    return _batches[res]


def render(cfg0, net, aggr, gb, thresh, r0, r1, S, shift=0.0):
    """One render of rays [r0, r1) with its own workspace -> the frame dict the checks read."""
    cfg = copy.deepcopy(cfg0)
    cfg.smpl_thresh = thresh
    cfg.aggr = aggr
    old = net.cfg
    net.cfg = cfg
    try:
        ctx = net.prepare(gb)
        ro, rd, nr, fa = (gb[k][0][r0:r1] for k in ('ray_o', 'ray_d', 'near', 'far'))
        if shift:
            nr = fa = fa + shift
        net._ws = None                                    # own workspace: the views must stay valid while the frame is cached
        out = net.render_rays(ctx, ro, rd, nr, fa, S, want_raw=True)
        sync()
        net._ws = None
    finally:
        net.cfg = old
    st = out['stats'].cpu()
    ws, n, S_, max_active = out['_ws']
    return dict(aggr=aggr, out=out, st=st, na=int(st[0]), n=n, S=S, ws=out['_ws'], v=_abi.ws_views(*out['_ws']), ctx=ctx, net=net,
                rays=tuple(_abi.f32c(t) for t in (ro, rd, nr, fa)), li=gb['latent_index'].reshape(-1)[:1].to(torch.int64).contiguous())


def render_occ(f):
    """The frame once more through invr_render_fwd itself with BOTH optional outputs raw and occ (Network.render_rays hands out occ as
    a view of raw's fourth channel), pre-filled with NaN -> raw (N,4), occ (N)."""
    L = _abi.lib()
    n, S, net, ctx = f['n'], f['S'], f['net'], f['ctx']
    ro, rd, nr, fa = f['rays']
    raw, occ = torch.full((n * S, 4), NAN, device=DEV), torch.full((n * S,), NAN, device=DEV)
    rgb, acc = torch.full((n, 3), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
    stats = torch.zeros(_abi.STATS_LEN, dtype=torch.int32, device=DEV)
    nbytes = L.invr_workspace_bytes(n, S, 0)
    ws = net.workspace(nbytes, ro.device)
    try:
        _abi.check(L.invr_render_fwd(C.byref(ctx.scene), C.byref(ctx.model), _abi.ptr(ro), _abi.ptr(rd), _abi.ptr(nr), _abi.ptr(fa), _abi.ptr(None),
                                     n, S, _abi.ptr(rgb), _abi.ptr(acc), _abi.ptr(raw), _abi.ptr(occ), _abi.ptr(None), _abi.ptr(None),
                                     _abi.ptr(stats, torch.int32), C.c_void_p(ws.data_ptr()), nbytes, 0, _abi.stream_ptr()))
        sync()
    finally:
        net._ws = None
    assert same_bits(rgb, f['out']['rgb_map']) and same_bits(acc, f['out']['acc_map'])
    return raw, occ


def frame(small_net, aggr, name, cached=True):
    """Frame `name` of the module docstring in merge mode `aggr` (rendered once per module unless cached=False)."""
    key = (aggr, name)
    if cached and key in _frames:
        return _frames[key]
    cfg0, net = small_net
    if name == 'C':
        gb, thresh = batch(48)
        f = render(cfg0, net, aggr, gb, thresh, 0, gb['ray_o'].shape[1], 96)
    else:
        gb, thresh = batch(G.RES)
        r0, r1 = A_RAYS or (0, gb['ray_o'].shape[1])
        if (DEV, A_RAYS) not in _trim:                    # the ragged flag-byte tail must be exercised: as check_list_groups trims
            n = r1
            na = render(cfg0, net, aggr, gb, thresh, r0, n, G.S)['na']
            while na % 8 == 0 and n > r1 - 64:
                n -= 1
                na = render(cfg0, net, aggr, gb, thresh, r0, n, G.S)['na']
            _trim[(DEV, A_RAYS)] = n
        r1 = _trim[(DEV, A_RAYS)]
        if name == 'B':
            r1 = r0 + 256
        f = render(cfg0, net, aggr, gb, thresh, r0, r1, G.S, shift=10.0 if name == 'D' else 0.0)
    f['name'] = name
    na = f['na']
    print('frame %s aggr %r: %d rays x %d samples, %d survivors (%d groups)' % (name, aggr, f['n'], f['S'], na, (max(na, 1) - 1) // GROUP + 1))
    assert int(f['st'][6]) == 0
    act = f['v']['active_idx'][:na].long()
    ray_major = torch.equal(act, act.sort()[0])
    if name == 'A':
        assert na > GROUP and na % 8 != 0, na
        assert A_RAYS is not None or na > 2 * GROUP, na
        assert not ray_major, 'frame A: the depth-windowed survivor order'
    elif name == 'B':
        assert 64 < na <= GROUP, na
    elif name == 'C':
        assert na > GROUP and f['S'] % 64 != 0 and ray_major, na
    else:
        assert na == 0, na
    if cached:
        _frames[key] = f
    return f


def merge_inputs(f):
    """What the merge of frame f saw, assembled from the workspace: listed, far (Na,5) bool, vals (Na,5,4) — the per-pair [rgb, occ] of
    the one-kernel part MLP on the frame's encoder outputs, asserted bit-identical to what the two phases stored —, pdist (Na,5),
    pair_of (Na,5) list index of every listed pair, cnt[5].  All on DEV; cached in the frame."""
    if 'inputs' in f:
        return f['inputs']
    v, na, aggr = f['v'], f['na'], f['aggr']
    L = _abi.lib()
    cap = v['cap']
    cnt = [int(f['st'][1 + p]) for p in range(5)]
    fl, ff = v['pflags'][:na].long(), v['farflags'][:na].long()
    listed = torch.stack([((fl >> p) & 1).bool() for p in range(5)], 1).reshape(na, 5)
    far = torch.stack([((ff >> p) & 1).bool() for p in range(5)], 1).reshape(na, 5)
    assert not bool((listed & far).any()), 'a (slot, part) is both listed and far'
    assert int(((fl | ff) >> 5).sum()) == 0
    vals = torch.full((na, 5, 4), NAN, device=DEV)
    pair_of = torch.full((na, 5), -1, dtype=torch.int64, device=DEV)
    pair_raw = []
    for p in range(5):
        n = cnt[p]
        assert n >= 1
        emb = v['emb'][p][:, :n].contiguous()
        d = v['l_d'][p][:, :n].contiguous()
        raw = torch.full((n, 4), NAN, device=DEV)
        count = torch.full((1,), n, dtype=torch.int32, device=DEV)
        _abi.check(L.invr_part_mlp_fwd(C.byref(f['ctx'].model), p, _abi.ptr(f['li'], torch.int64), _abi.ptr(emb), _abi.ptr(d), n,
                                       _abi.ptr(count, torch.int32), _abi.ptr(raw), _abi.stream_ptr()))
        sync()
        assert not bool(torch.isnan(raw).any())
        slots = v['l_slot'][p][:n].long()
        assert int(slots[-1]) == cap, 'the far-constant pair closes the list, at slot cap'
        assert torch.equal(slots[:-1], listed[:, p].nonzero(as_tuple=True)[0]), p      # every listed pair once, ascending
        # both phases reproduce the one-kernel results bit for bit (csrc/k_mlp.hip header)
        assert same_bits(v['occp'][p][:n], raw[:, 3]), ('occp', p, int((bits(v['occp'][p][:n]) != bits(raw[:, 3])).sum()))
        if aggr in ('mean', 'dist'):
            feat = v['feat'][p][0:4 * n:4]
            assert same_bits(feat, raw), ('feat', p, int((bits(feat) != bits(raw)).any(1).sum()))
        vals[slots[:-1], p] = raw[:-1]
        vals[far[:, p], p] = raw[-1]
        pair_of[slots[:-1], p] = torch.arange(n - 1, device=DEV)
        pair_raw.append(raw)
    pdist = v['pdist'][:na].clone() if aggr in ('dist', 'mindist') else torch.zeros(na, 5, device=DEV)
    f['inputs'] = dict(listed=listed, far=far, vals=vals, pdist=pdist, pair_of=pair_of, cnt=cnt, pair_raw=pair_raw)
    return f['inputs']


def reference(f):
    if 'ref' not in f:
        i = merge_inputs(f)
        f['ref'] = MG.merge(f['aggr'], i['listed'].cpu(), i['far'].cpu(), i['vals'].cpu(), i['pdist'].cpu())
    return f['ref']


def record(case, K, k_allowed):
    HEADROOM[case] = K
    print('%-40s K = %.3f   (allowed %.1f)' % (case, K, k_allowed / 2.0))


def check_sum(got, ref, k, case):
    """|got - exact| <= k 2^-24 A + c 2^-126 per element; NaN where exact is NaN; A == 0 requires exactly 0.0."""
    got = got.cpu().double()
    exact, A = ref.exact, ref.A
    c = ref.c if torch.is_tensor(ref.c) else torch.tensor(float(ref.c), dtype=torch.float64)
    c = c.reshape(-1, *([1] * (exact.dim() - 1))) if c.dim() else c
    nan = torch.isnan(exact)
    assert torch.equal(torch.isnan(got), nan), (case, 'NaN pattern')
    err = torch.where(nan, torch.zeros_like(exact), (got - exact).abs())
    A_ = torch.where(nan, torch.zeros_like(A), A)
    assert bool((got[(A_ == 0) & ~nan] == 0).all()), (case, 'A == 0 requires exactly 0.0')
    K = float((err / (2 * U * A_).clamp_min(1e-300))[A_ > 0].max()) if bool((A_ > 0).any()) else 0.0
    record(case, K, k)
    bad = err > k * U * A_ + c * TINY
    assert not bool(bad.any()), (case, int(bad.sum()), K)


def check_forward(f):
    """Everything the merge of frame f wrote, per survivor."""
    v, na, aggr, st = f['v'], f['na'], f['aggr'], f['st']
    i = merge_inputs(f)
    m = reference(f)
    cnt, lc = i['cnt'], v['lcap']
    g_last = (max(na, 1) - 1) // GROUP
    wsel = v['wsel'][:na].long()
    assert torch.equal(wsel.cpu(), m.wsel), (aggr, int((wsel.cpu() != m.wsel).sum()))
    wcnt = v['wcnt'][:g_last + 1].long()
    rgbw = v['rgbw']
    if aggr in ('', 'mindist'):
        # the merged value = the selected value, bit for bit: rgbw[slot] for a listed winner, rgbw[lcap + p] for a far one, zeros for none
        part = (wsel % 8).clamp_max(4)
        merged = torch.where((wsel < 5)[:, None], rgbw[:na], torch.where((wsel < 16)[:, None], rgbw[lc + part], torch.zeros(na, 4, device=DEV)))
        assert same_bits(merged.cpu(), m.exact.float()), (aggr, int((bits(merged.cpu()) != bits(m.exact.float())).any(1).sum()))
        for p in range(5):
            assert same_bits(rgbw[lc + p], i['pair_raw'][p][-1]), ('far constant', p)
        # wl / wcnt: exactly the listed winners (+ the far-constant pair of every part), segment by segment
        for p in range(5):
            real = v['l_slot'][p][:cnt[p] - 1].long()
            want = (wsel == p).nonzero(as_tuple=True)[0]
            exp_cnt = torch.bincount(want // GROUP, minlength=g_last + 1)
            exp_cnt[g_last] += 1
            assert torch.equal(wcnt[:, p], exp_cnt), (aggr, p)
            got = P.winner_list_entries(v['wl'][p], wcnt[:, p], real, g_last)
            assert int(got[-1]) == cnt[p] - 1
            assert torch.equal(got[:-1], i['pair_of'][want, p]), (aggr, p)
    else:
        # every pair "wins": wcnt = gcount (+ the far-constant pair in the last group's row), wl = the identity
        exp = v['gcount'][:g_last + 1].long().clone()
        exp[g_last] += 1
        assert torch.equal(wcnt, exp), (aggr, wcnt.tolist(), exp.tolist())
        for p in range(5):
            per_group = torch.bincount(v['l_slot'][p][:cnt[p] - 1].long() // GROUP, minlength=g_last + 1)
            assert torch.equal(v['gcount'][:g_last + 1, p].long(), per_group), p
            assert torch.equal(v['wl'][p][:cnt[p]].long(), torch.arange(cnt[p], device=DEV)), p
        check_sum(rgbw[:na], m, K_FWD[aggr], 'fwd %s frame %s' % (aggr, f['name']))
        merged = torch.where((wsel == 0)[:, None], rgbw[:na], torch.zeros(na, 4, device=DEV))
    # the scatter: raw[active_idx[slot]] = the merged value, bit for bit; every other row exactly zero
    raw = f['out']['raw']
    N = f['n'] * f['S']
    assert raw.shape == (N, 4)
    act = v['active_idx'][:na].long()
    assert na == 0 or (int(act.min()) >= 0 and int(act.max()) < N)
    assert int(torch.unique(act).numel()) == na
    assert same_bits(raw[act], merged), (aggr, int((bits(raw[act]) != bits(merged)).any(1).sum()))
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[act] = False
    assert bool((raw[rest] == 0).all())
    assert torch.equal(f['out']['occ'], raw[:, 3])
    if f['name'] in ('B', 'D'):                           # ... and the library's own occ output: raw's fourth channel, every row written
        raw2, occ2 = render_occ(f)
        assert same_bits(raw2, raw) and same_bits(occ2, raw[:, 3]), aggr
    if na == 0:
        for k in ('rgb_map', 'acc_map', 'raw'):
            assert bool((f['out'][k] == 0).all()), k
        assert [int(x) for x in st[1:6]] == [1] * 5


def census(f):
    """-> the number of survivors of every class the merge kernels tell apart."""
    i = merge_inputs(f)
    m = reference(f)
    listed, far = i['listed'].cpu(), i['far'].cpu()
    c = {'two or more listed parts': int((listed.sum(1) >= 2).sum()),
         'far only': int((far.any(1) & ~listed.any(1)).sum()),
         'no flagged part': int((~(listed | far).any(1)).sum())}
    if f['aggr'] == 'mindist':
        # (part_dist is what flags a part: the part of smallest part_dist is unflagged only where no part is flagged)
        c['the minimum-distance part is unflagged'] = int((m.wsel == 255).sum())
    if f['aggr'] == '':
        c['a far constant wins'] = int(((m.wsel >= 8) & (m.wsel < 13)).sum())
    return c


def run_merge_bwd(f, g_full):
    """invr_merge_bwd on the workspace of frame f -> g_raws (lcap*5,4) on the CPU, the must-not-touch rows already asserted."""
    v, na = f['v'], f['na']
    ws, n, S, max_active = f['ws']
    cap, lc = v['cap'], v['lcap']
    g_raws = torch.full((lc * 5, 4), MARK, dtype=torch.int32).view(torch.float32)
    g_raws[:na * 5] = NAN
    g_raws[cap * 5:] = NAN                                 # the far row: the call clears it itself (include/invr.h)
    g_raws = g_raws.to(DEV)
    g_dev = g_full.to(DEV).contiguous()
    _abi.check(_abi.lib().invr_merge_bwd(AGGR_CODE[f['aggr']], C.c_void_p(ws.data_ptr()), ws.numel(), n, S, max_active,
                                         _abi.ptr(g_dev), _abi.ptr(g_raws), _abi.stream_ptr()))
    sync()
    g_raws = g_raws.cpu()
    assert bool((bits(g_raws[na * 5:cap * 5]) == MARK).all()), 'rows of slots [Na, cap): written where nothing may be written'
    return g_raws


def check_transpose(f, case, seed=0):
    """invr_merge_bwd on what the workspace of frame f holds NOW (the frame's own state, or a synthetic one written over it)."""
    v, na, aggr = f['v'], f['na'], f['aggr']
    cap = v['cap']
    N = f['n'] * f['S']
    g_full = torch.randn(N, 4, generator=torch.Generator().manual_seed(seed))
    got = run_merge_bwd(f, g_full)
    fl, ff = v['pflags'][:na].long().cpu(), v['farflags'][:na].long().cpu()
    listed = torch.stack([((fl >> p) & 1).bool() for p in range(5)], 1).reshape(na, 5)
    far = torch.stack([((ff >> p) & 1).bool() for p in range(5)], 1).reshape(na, 5)
    pdist = v['pdist'][:na].cpu() if aggr in ('dist', 'mindist') else torch.zeros(na, 5)
    g = g_full[v['active_idx'][:na].long().cpu()]
    exact, far_rows = MG.merge_bwd(aggr, listed, far, v['wsel'][:na].cpu(), pdist, g)
    per = got[:na * 5].view(na, 5, 4)
    assert not bool(torch.isnan(per).any()), (case, 'an entry of a survivor was not written')
    if aggr in ('', 'mindist'):
        # the listed winner's entry is a bit copy of g, every other entry +0.0
        assert same_bits(per, exact.float()), (case, int((bits(per) != bits(exact.float())).any(2).sum()))
        on = torch.zeros(na, 5, dtype=torch.bool)
    else:
        on = listed
        assert bool((per[~on] == 0).all()), (case, 'a part that is not listed received a gradient')
        A = exact.abs()
        check_sum(per[on], MG.Ref(exact[on], A[on], 0.0), K_BWD[aggr], 'bwd %s' % case)
    n_far = 0
    for p in range(5):
        r = far_rows[p]
        row = got[cap * 5 + p].double()
        assert not bool(torch.isnan(row).any()), (case, p, 'the far row was not cleared')
        if r.c == 0:
            assert bool((bits(got[cap * 5 + p]) == 0).all()), (case, p)
            continue
        n_far += int(r.c)
        err = (row - r.exact).abs()
        K = float((err / (2 * U * r.A).clamp_min(1e-300)).max())
        record('bwd %s far row %d (n = %d)' % (case, p, int(r.c)), K, r.c + 4)
        assert bool((err <= (r.c + 4) * U * r.A).all()), (case, p, int(r.c), K)
    return n_far, int(on.sum())


def synthetic_states(na, aggr, seed):
    """-> [(name, wsel, pflags, farflags, pdist or None)]: valid states only (wsel codes 0-4, 8-12, 255; never a flag bit and its far
    bit together), the select and the sum flows' inputs consistent with each other."""
    g = torch.Generator().manual_seed(seed)
    u8 = lambda x: torch.full((na,), x, dtype=torch.uint8)
    states = [('every survivor far for part 3', u8(8 + 3), u8(0), u8(1 << 3), None),
              ('every survivor WSEL_NONE', u8(255), u8(0), u8(0), None),
              ('all five parts listed', torch.randint(0, 5, (na,), generator=g).to(torch.uint8) if aggr in ('', 'mindist') else u8(0),
               u8(0x1f), u8(0), None)]
    if aggr == 'dist':
        kind = torch.randint(0, 3, (na, 5), generator=g)                   # 0 unflagged, 1 listed, 2 far
        pf = sum(((kind[:, p] == 1).long() << p) for p in range(5)).to(torch.uint8)
        ff = sum(((kind[:, p] == 2).long() << p) for p in range(5)).to(torch.uint8)
        pd = torch.rand(na, 5, generator=g) * 0.5
        special = torch.randint(0, 6, (na, 5), generator=g)
        pd[special == 0] = 0.0
        pd[special == 1] = 2.0 ** -140                                       # a float32 denormal
        pd[special == 2] = float('inf')
        pd[0] = 0.0
        pd[1 % na] = float('inf')                                            # every weight 0: the clamped norm
        states.append(('pdist with 0, a denormal and +inf', torch.where(kind.ne(0).any(1), 0, 255).to(torch.uint8), pf, ff, pd))
    return states


@pytest.fixture(scope='module')
def small_net():
    return G.make_small_net(DEV)


@pytest.mark.parametrize('name', FRAMES)
@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_merge_forward_per_survivor(small_net, aggr, name):
    check_forward(frame(small_net, aggr, name))


@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_frame_a_holds_every_class(small_net, aggr):
    c = census(frame(small_net, aggr, 'A'))
    print('aggr %r:' % aggr, c)
    for k, n in c.items():
        assert n >= CENSUS_MIN, (aggr, k, n)


@pytest.mark.parametrize('name', ('A', 'B', 'D'))
@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_merge_bwd_on_frame(small_net, aggr, name):
    f = frame(small_net, aggr, name)
    n_far, n_on = check_transpose(f, '%s frame %s' % (aggr or 'max', name), seed=3)
    if name == 'A' and A_RAYS is None:
        assert n_far >= CENSUS_MIN and (n_on >= CENSUS_MIN or aggr in ('', 'mindist'))
    if name == 'D':
        assert n_far == 0 and n_on == 0


@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_merge_bwd_synthetic_states(small_net, aggr):
    """The transpose reads counters, active_idx, wsel, pflags, farflags and pdist, nothing else: states written over frame B's."""
    f = frame(small_net, aggr, 'B', cached=False)
    v, na = f['v'], f['na']
    for k, (case, wsel, pf, ff, pd) in enumerate(synthetic_states(na, aggr, seed=5)):
        assert not bool((pf & ff).any())
        v['wsel'][:na] = wsel.to(DEV)
        v['pflags'][:na] = pf.to(DEV)
        v['farflags'][:na] = ff.to(DEV)
        if pd is not None:
            v['pdist'][:na] = pd.to(DEV)
        n_far, n_on = check_transpose(f, '%s %s' % (aggr or 'max', case), seed=10 + k)
        if case.startswith('every survivor far'):
            assert n_far == na
        if case.startswith('every survivor WSEL_NONE'):
            assert n_far == 0 and n_on == 0
        if case.startswith('all five'):
            assert n_far == 0 and n_on == (0 if aggr in ('', 'mindist') else 5 * na)
