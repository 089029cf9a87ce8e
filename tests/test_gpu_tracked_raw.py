"""GPU: invr_render_fwd_tracked (include/invr.h) — renders into a caller-owned raw buffer whose zero rows are tracked by one dirty bit per
row instead of being rewritten every frame.  Whatever the buffer held before, the first N = n_rays * n_samples rows, rgb_map and
acc_map are bit for bit what the untracked call gives, every row whose bit is clear holds zeros, and nothing at or beyond N is touched.
S = 64 / 128 take the word-wise kernel (k_composite_words: stores only `cur | prev`, skips empty passes and empty rays), S = 32 / 96 the
dense stores with the follow-up launch that brings the dirty words to the mask.  The bodies run on the host build of the kernels in
tests/test_hostsim_tracked_raw_cpu.py; the untracked reference renders are made once per (S, res, frame) and shared.
For S a multiple of 64 the untracked render runs the same word-wise kernel, so every reference is itself checked against a kernel this
path shares nothing with: its raw goes through invr_composite_fwd (k_composite<DenseRaw>: every pass of every ray computed, the same
per-lane arithmetic) and the maps must come out bit for bit.  cfg.random_bg (epsilon 1: empty passes are NOT the identity and must be
computed) has a case of its own, checked against a float64 evaluation of the compositing."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
FAST, FALLBACK = (64, 128), (32, 96)
_NETS, _FRAMES, _REFS = {}, {}, {}


def _net(S, random_bg=False):
    if (DEV, S, random_bg) not in _NETS:
        import invr  # noqa: F401
        from invr import params
        from invr.config import make_cfg
        from invr.network import Network
        cfg = make_cfg(table_log2=12, N_samples=S, random_bg=random_bg)
        net = Network(cfg=cfg)
        net.load_state_dict(params.init_state_dict(cfg, seed=4), strict=True)
        _NETS[(DEV, S, random_bg)] = net.to(DEV).eval()
    return _NETS[(DEV, S, random_bg)]


def _frame(res, k):
    """-> (batch on DEV, (ray_o, ray_d, near, far))"""
    if (DEV, res, k) not in _FRAMES:
        from invr import scene
        b, _ = scene.make_scene(res, res, seed=0, cam_dist=1.8, frame=3 + 7 * k, pose_seed=k)
        b = {kk: v.to(DEV) for kk, v in scene.to_torch(b).items()}
        _FRAMES[(DEV, res, k)] = (b, tuple(b[key][0].contiguous() for key in ('ray_o', 'ray_d', 'near', 'far')))
    return _FRAMES[(DEV, res, k)]


def _render(S, res, k, rays=None, random_bg=False, **kw):
    net = _net(S, random_bg)
    b, a = _frame(res, k)
    a = rays or a
    net._ws = None
    out = net.render_rays(b, a[0], a[1], a[2], a[3], S, want_raw=True, **kw)
    net._ws = None
    return out


def _dense_maps(raw, S):
    """rgb_map, acc_map of a raw tensor by invr_composite_fwd: the dense kernel (epsilon 0), every pass of every ray"""
    from invr import _abi
    n = raw.shape[0] // S
    rgb, acc = torch.empty(n, 3, device=raw.device), torch.empty(n, device=raw.device)
    _abi.check(_abi.lib().invr_composite_fwd(_abi.ptr(raw.contiguous()), n, S, _abi.ptr(None), _abi.ptr(rgb), _abi.ptr(acc), _abi.stream_ptr()))
    return rgb, acc


def _check_against_dense_kernel(o, S):
    rgb, acc = _dense_maps(o['raw'], S)
    assert torch.equal(rgb.view(torch.int32), o['rgb_map'].view(torch.int32)), 'rgb_map differs from the dense compositing of the same raw'
    assert torch.equal(acc.view(torch.int32), o['acc_map'].view(torch.int32)), 'acc_map differs from the dense compositing of the same raw'


def _ref(S, res, k, max_active=0, random_bg=False):
    """the untracked render of frame k (made once, never modified)"""
    key = (DEV, S, res, k, max_active, random_bg)
    if key not in _REFS:
        o = _render(S, res, k, max_active=max_active, random_bg=random_bg)
        _REFS[key] = {kk: o[kk].clone() for kk in ('rgb_map', 'acc_map', 'raw', 'stats')}
        if not random_bg:
            _check_against_dense_kernel(_REFS[key], S)
    return _REFS[key]


def _bits(dirty, rows):
    """(rows,) bool: the dirty bit of every row"""
    sh = torch.arange(64, device=dirty.device, dtype=torch.int64)
    return (((dirty[:, None] >> sh) & 1) != 0).reshape(-1)[:rows]


def _pair(rows, poisoned):
    if poisoned:
        return (torch.full((rows * 4,), float('nan'), device=DEV), torch.full((-(-rows // 64),), -1, device=DEV, dtype=torch.int64))
    return torch.zeros(rows * 4, device=DEV), torch.zeros(-(-rows // 64), device=DEV, dtype=torch.int64)


def _tracked_and_checked(S, res, k, raw, dirty, max_active=0, rays=None, ref=None, random_bg=False):
    """One tracked render of frame k into (raw, dirty) with every check of the contract -> (output, bits before, bits after)."""
    rows = raw.numel() // 4
    raw_before, before = raw.clone(), _bits(dirty, rows)
    # the precondition of the call: a row whose bit is clear holds four +0.0f
    assert bool((raw.view(torch.int32).view(rows, 4)[~before] == 0).all())
    out = _render(S, res, k, rays=rays, max_active=max_active, random_bg=random_bg, raw_out=raw, raw_dirty=dirty)
    ref = ref or _ref(S, res, k, max_active, random_bg)
    N = ref['raw'].shape[0]
    assert N <= rows and out['raw'].shape == ref['raw'].shape and out['raw'].data_ptr() == raw.data_ptr()
    for key in ('raw', 'rgb_map', 'acc_map'):
        assert torch.equal(out[key].view(torch.int32), ref[key].view(torch.int32)), (S, res, k, key)
    assert torch.equal(out['occ'], ref['raw'][:, 3]) and torch.equal(out['stats'], ref['stats'])
    after = _bits(dirty, rows)
    words = raw.view(torch.int32).view(rows, 4)
    assert bool((words[~after] == 0).all()), 'a row whose dirty bit is clear is not zero'
    assert bool(after[:N][(ref['raw'].view(torch.int32) != 0).any(1)].all()), 'a non-zero row is not marked dirty'
    assert torch.equal(after[N:], before[N:]), 'dirty bits at or beyond N changed'
    assert torch.equal(words[N:], raw_before.view(torch.int32).view(rows, 4)[N:]), 'rows at or beyond N changed'
    return out, before, after


def body_sequence(S, res):
    refs = [_ref(S, res, k) for k in range(3)]
    Ns = [r['raw'].shape[0] for r in refs]
    assert len(set(Ns)) == 3, 'the three poses have different ray counts'
    rows = int(1.05 * max(Ns))
    raw, dirty = _pair(rows, poisoned=False)
    stale = empty_word = empty_ray = straddle = False
    for k in (1, 0, 2, 1):          # (a shorter frame after a longer one: its tail stays dirty beyond N)
        out, before, after = _tracked_and_checked(S, res, k, raw, dirty)
        N, n = Ns[k], Ns[k] // S
        stale |= bool((before[:N] & ~after[:N]).any())                       # dirty only from the frame before: cleaned by this one
        live = after[:N].view(n, S)
        empty_ray |= bool((~live.any(1)).any()) and bool(live.any(1).any())
        w = after[:N - N % 64].view(-1, 64).any(1)
        empty_word |= bool((~w).any()) and bool(w.any())
        if S % 64 == 0 and S > 64:
            passes = live.view(n, S // 64, 64).any(2)
            straddle |= bool((passes.any(1) & ~passes.all(1)).any())
    # the frames exercise what the kernel distinguishes (checked on the host build before the GPU run)
    assert stale and empty_word and empty_ray
    assert straddle or S % 64 != 0 or S == 64


def body_poisoned(S, res):
    N = _ref(S, res, 0)['raw'].shape[0]
    rows = int(1.05 * N)
    raw, dirty = _pair(rows, poisoned=True)
    out, before, after = _tracked_and_checked(S, res, 0, raw, dirty)
    assert bool(before.all()) and bool(after[N:].all()) and not bool(after[:N].all())
    assert bool(torch.isnan(raw.view(rows, 4)[N:]).all()) and not bool(torch.isnan(out['raw']).any())
    _tracked_and_checked(S, res, 1, raw, dirty)          # ... and the pair goes on from there


def body_undersized(S, res):
    na = int(_ref(S, res, 0)['stats'][0])
    assert na > 1000
    cap = na // 2
    ref = _ref(S, res, 0, max_active=cap)
    assert int(ref['stats'][6]) != 0
    rows = int(1.05 * ref['raw'].shape[0])
    raw, dirty = _pair(rows, poisoned=False)
    _tracked_and_checked(S, res, 1, raw, dirty)                                   # leaves rows dirty for the truncated frame to clean
    out, _, _ = _tracked_and_checked(S, res, 0, raw, dirty, max_active=cap)
    assert int(out['stats'][6]) != 0
    assert not torch.equal(out['rgb_map'], _ref(S, res, 0)['rgb_map'])           # (the truncation does show)


def body_empty(S, res):
    b, a = _frame(res, 0)
    away = (a[3] + 10.0).contiguous()                    # near = far, ten metres behind the body box: no sample survives the cull
    rays = (a[0], a[1], away, away)
    N = a[0].shape[0] * S
    rows = int(1.05 * N)
    raw, dirty = _pair(rows, poisoned=False)
    _tracked_and_checked(S, res, 0, raw, dirty)
    assert bool(_bits(dirty, rows)[:N].any())
    ref = _render(S, res, 0, rays=rays)
    ref = {kk: ref[kk].clone() for kk in ('rgb_map', 'acc_map', 'raw', 'stats')}
    _check_against_dense_kernel(ref, S)
    assert int(ref['stats'][0]) == 0
    out, _, after = _tracked_and_checked(S, res, 0, raw, dirty, rays=rays, ref=ref)
    for key in ('rgb_map', 'acc_map', 'raw'):
        assert bool((out[key].view(torch.int32) == 0).all()), key
    assert not bool(after.any()) and bool((raw.view(torch.int32) == 0).all())          # fully cleaned


def body_random_bg(S, res):
    """cfg.random_bg: epsilon = 1, a pass without a survivor multiplies the transmittance by 2^64 — nothing may be skipped.  Tracked
    against untracked bit for bit (from a dirty pair), and both against the compositing in float64.  Bound: a factor 1 - alpha + eps
    carries two roundings and every multiply of the product scan one, so a weight of sample s is off by at most (3 s + 2) u relatively,
    u = 2^-24; the per-lane fmaf over the passes and the six-level wave sum add at most (S / 64 + 6) u.  All terms are non-negative,
    so the maps are within (3 S + 12) u of their float64 values, relatively."""
    ref = _ref(S, res, 0, random_bg=True)
    N = ref['raw'].shape[0]
    n = N // S
    raw, dirty = _pair(int(1.05 * N), poisoned=False)
    _tracked_and_checked(S, res, 1, raw, dirty, random_bg=True)
    out, _, after = _tracked_and_checked(S, res, 0, raw, dirty, random_bg=True)
    live = after[:N].view(n, S // 64, 64).any(2)
    assert bool((~live).any()) and bool(live.any())                      # there are empty passes: the skip would have applied
    r = ref['raw'].double().view(n, S, 4)
    alpha = r[..., 3]
    T = torch.cumprod(1.0 - alpha + 1.0, 1)
    T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], 1)
    w = alpha * T
    acc, rgb = w.sum(1), (w[..., None] * r[..., :3]).sum(1)
    assert bool(torch.isfinite(out['acc_map']).all()) and float(acc.max()) > 1.5          # (far beyond what epsilon 0 can give)
    tol = (3 * S + 12) * 2.0 ** -24
    assert bool(((out['acc_map'].double() - acc).abs() <= tol * acc + 1e-30).all())
    assert bool(((out['rgb_map'].double() - rgb).abs() <= tol * rgb + 1e-30).all())
    # ... and it is not what epsilon 0 gives for the same raw
    assert not torch.equal(_dense_maps(ref['raw'], S)[1], out['acc_map'])


def test_tracked_entry_refuses_occ_weights_and_a_short_buffer():
    import ctypes as C
    from invr import _abi
    L = _abi.lib()
    assert L.invr_raw_dirty_bytes(1) == 8 and L.invr_raw_dirty_bytes(64) == 8 and L.invr_raw_dirty_bytes(65) == 16 and L.invr_raw_dirty_bytes(0) == 0
    one = C.c_void_p(256)
    none = C.c_void_p(0)
    head = (None, None, none, none, none, none, none, 4, 64, one, one, one)
    tail = (none, none, none, 0, 0, none)
    assert L.invr_render_fwd_tracked(*head, one, none, *tail, one, 4 * 64) != 0 and b'occ' in L.invr_last_error()
    assert L.invr_render_fwd_tracked(*head, none, one, *tail, one, 4 * 64) != 0 and b'weights' in L.invr_last_error()
    assert L.invr_render_fwd_tracked(*head, none, none, *tail, one, 4 * 64 - 1) != 0 and b'raw_rows' in L.invr_last_error()
    assert L.invr_render_fwd_tracked(*head, none, none, *tail, none, 4 * 64) != 0 and b'raw_dirty' in L.invr_last_error()


CASES = [(S, res) for S in FAST + FALLBACK for res in (64, 128)]
RAY_MAJOR = 192          # a multiple of 64 that is no power of two: the word-wise kernel on ray-major survivor ranks, three passes per ray


@pytest.mark.parametrize('S,res', CASES + [(RAY_MAJOR, 64)])
def test_sequence_of_three_poses_into_one_pair(S, res):
    body_sequence(S, res)


@pytest.mark.parametrize('S,res', CASES)
def test_poisoned_start(S, res):
    body_poisoned(S, res)


@pytest.mark.parametrize('S,res', CASES)
def test_undersized_max_active(S, res):
    body_undersized(S, res)


@pytest.mark.parametrize('S,res', CASES)
def test_empty_frame_cleans_the_buffer(S, res):
    body_empty(S, res)


@pytest.mark.parametrize('S', FAST)
def test_random_bg_epsilon_computes_the_empty_passes(S):
    body_random_bg(S, 64)
