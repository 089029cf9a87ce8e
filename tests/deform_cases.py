"""Test infrastructure shared by the deformer-backward tests (tests/test_deform_reference_cpu.py, tests/test_gpu_deform_bwd.py and its
wave-machine twin): grid specs, a synthetic UV volume, seeded tables and weight sets, point clouds, upstream-gradient patterns, the
per-element noise scale and the acceptance rule.  Checker only: oracle.nvr_oracle and the float64 references; no kernel is reached
from here and nothing of the product is imported.

The rule is EC.accept, unchanged, every element judged, none left out:
    |kernel - exact| <= 8 noise + (c + 4) 2^-24 A + c 2^-126,        A == 0 requires exactly 0.0
(on the `faces` cloud with the `touched` convention of tests/test_gpu_encoder_bwd.py for the table gradients: a row that the exact,
a perturbed or the fp32 evaluation reaches need not be exactly 0).  noise per element = the largest of
  (a) the deviation from `exact` of torch's fp32 autograd of the oracle's deformer on the CPU (oracle.nvr_oracle.deformer's own
      operations, restated step by step so that the per-entry matrices can be read off; asserted bit-identical to it on the first 8192 entries of a case),
  (b) the largest move of `exact` under 4 sign-random perturbations of the inputs: pts by (|x| + 1) 2^-23, g_resd by |g| 2^-23 (zero
      rows stay zero).  A point has three coordinates, so only four sign patterns differ by more than a global sign: every entry gets
      all four, in a random order and each with a random global sign.  (Four independent draws repeat a pattern more often than not,
      and the moves an entry's three coordinates cause can cancel under one pattern: among 1e5 elements some would be left with a
      noise far below their first-order sensitivity to any single coordinate.)
  (c) the largest move of `exact` under 4 sign-random draws of the VALUE error csrc/common.h documents for softplus_f: every forward
      Softplus output by +-max(1 fp32 ulp of itself, 1.5e-7).  Values only: the reference's derivative factors stay computed from z.
Nothing is fitted to a kernel.  Inputs are evaluated in chunks of CHUNK entries (the per-entry outputs are independent of each other;
the parameter gradients add up over the chunks), so that the largest cases need no more memory than the small ones."""
import functools

import torch
import torch.nn.functional as F

from oracle import nvr_oracle as O
from tests import deform_reference as DR
from tests import encoder_cases as EC
from tests import grid_reference as GR
from tests import mlp_cases as MC
from tests.mlp_reference import Ref

N_BASE = 5000                      # the seeded base batch; a case of n <= N_BASE entries takes its first n rows
CHUNK = 32768
WEIGHT_SETS = ('init', 'wide', 'saturated-head')
CLOUDS = ('inside', 'outside', 'nodes', 'one', 'faces')
PATTERNS = ('dense', 'sparse')
FRAMES = {'t0': 0.0, 'tmid': 0.37, 't1': 1.0}          # normalised t = 0 / interior / 1 (t1: c0z == c1z, both weights add into one row)
BBOX = [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]              # the deformer grid's bounds (config.DEFAULTS: the embedder's default box)
SPECS = {'prod': EC.SPECS['deformer'],                 # config.DEFAULTS tpose_deformer (pinned in the GPU module): slices 2959 float2
         'fallback': dict(EC.SPECS['deformer-small'], include_input=True)}      # res 4 .. 68: slices 8251 float2 > DF_SLICE_MAX
# the synthetic UV volume: unequal dims with D - 1 a power of two and power-of-two extents, so that a voxel node's coordinate, its
# normalised position and with them the sampled value are EXACT in fp32 and float64 alike (the `nodes` and `faces` clouds)
TUV_DIMS = (9, 5, 17)
TBOUNDS = [[-1.0, -0.5, -2.0], [1.0, 0.5, 2.0]]
N_SPECIAL = 160                    # nodes whose (u, v) sits on level-cell boundaries / on 0 and 1 (the `faces` cloud)


def make_spec(tag):
    return O.embedder_geometry(bbox=BBOX, **SPECS[tag])


def node_xyz(idx):
    """(m,3) integer node indices -> world coordinates (exact in fp32)."""
    b = torch.tensor(TBOUNDS, dtype=torch.float64)
    d = torch.tensor(TUV_DIMS, dtype=torch.float64) - 1.0
    return (b[0] + idx.double() * (b[1] - b[0]) / d).float()


@functools.lru_cache(maxsize=None)
def make_volume(tag):
    """-> (tuv (9,5,17,2) float32 in [0.02, 0.98], special (N_SPECIAL,3) node indices).  The special nodes carry u and / or v exactly on a
    level-cell boundary k * cell_l of the spec (as fp32 forms it), or exactly 0 or 1."""
    spec = make_spec(tag)
    g = torch.Generator().manual_seed(900 + sum(map(ord, tag)))
    tuv = torch.rand(*TUV_DIMS, 2, generator=g) * 0.96 + 0.02
    flat = torch.randperm(TUV_DIMS[0] * TUV_DIMS[1] * TUV_DIMS[2], generator=g)[:N_SPECIAL]
    special = torch.stack([flat // (TUV_DIMS[1] * TUV_DIMS[2]), (flat // TUV_DIMS[2]) % TUV_DIMS[1], flat % TUV_DIMS[2]], 1)
    for j in range(N_SPECIAL):
        for a in range(2):
            kind = int(torch.randint(0, 4, (1,), generator=g))
            if kind == 0 and a == 1:
                continue                                            # (v stays generic: only u on a boundary)
            if kind == 1:
                val = float(torch.randint(0, 2, (1,), generator=g))                                   # exactly 0 or 1
            else:
                l = int(torch.randint(0, spec['L'], (1,), generator=g))
                k = int(torch.randint(1, int(spec['res'][l]) - 1, (1,), generator=g))
                val = float((torch.tensor(float(k)) * spec['size'][l]).float())                       # k * cell_l, rounded as fp32 does
            tuv[special[j, 0], special[j, 1], special[j, 2], a] = val
    return tuv.contiguous(), special


@functools.lru_cache(maxsize=None)
def make_tables(tag):
    """Seeded ~N(0, 0.1^2) tables -> (dense (dense_rows,2), hash (n_hash,T,2))."""
    sp = make_spec(tag)
    assert sp['separate_dense']
    g = torch.Generator().manual_seed(40 + sum(map(ord, tag)))
    return torch.randn(sp['dense_rows'], 2, generator=g) * 0.1, torch.randn(sp['n_hash'], sp['T'], 2, generator=g) * 0.1


def make_scene(tag, frame):
    return dict(tuv=make_volume(tag)[0], tbounds=torch.tensor(TBOUNDS), frame_dim=torch.tensor(FRAMES[frame], dtype=torch.float32))


def tie_mask(uvt, spec):
    """GR.tie_mask's definition with a four times wider band (2^-18: here (u, v) is itself a computed value, good to a few fp32 ulp) and
    coordinates exactly on 0 or 1 always exempt (frame_dim is on a face of the box by design)."""
    xn = GR.normalise(uvt, spec['bbox'])
    drop = torch.zeros(uvt.shape[0], dtype=torch.bool)
    for l in range(spec['L']):
        res = int(spec['res'][l])
        q = xn / spec['size'][l].double()
        tie = (q > -1.5) & (q < res + 0.5) & ((q - q.round()).abs() <= 2.0 ** -18 * q.abs().clamp(min=1.0))
        drop |= (tie & ~((xn == 0.0) | (xn == 1.0))).any(1)
    return drop


@functools.lru_cache(maxsize=8)
def make_cloud(kind, n, tag='prod', frame='tmid'):
    """-> pts (n,3) float32.  n <= N_BASE: the first n rows of the N_BASE cloud.  Entries whose (u, v, t) lies on a cell tie are removed
    by the float64 reference alone and before anything runs (not on `faces`, whose ties are its purpose)."""
    if n < N_BASE:
        return make_cloud(kind, N_BASE, tag, frame)[:n].contiguous()
    spec = make_spec(tag)
    scene = make_scene(tag, frame)
    b = torch.tensor(TBOUNDS, dtype=torch.float64)
    dims = torch.tensor(TUV_DIMS)
    for attempt in range(8):
        g = torch.Generator().manual_seed(5000 + 31 * CLOUDS.index(kind) + attempt + (0 if n == N_BASE else n))
        m = n + max(4096, n // 8)
        u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
        if kind == 'inside':
            x = (b[0] + u(m, 3) * (b[1] - b[0])).float()
        elif kind == 'outside':                                     # beyond the bounds on EVERY axis: the border clamp, 8 corner nodes
            side = torch.randint(0, 2, (m, 3), generator=g).double()
            x = (b[0] + (side + (2.0 * side - 1.0) * (0.01 + u(m, 3))) * (b[1] - b[0])).float()
        elif kind == 'nodes':
            x = node_xyz(torch.stack([torch.randint(0, int(dims[a]), (m,), generator=g) for a in range(3)], 1))
        elif kind == 'one':
            x = (b[0] + u(1, 3) * (b[1] - b[0])).float().expand(m, 3).contiguous()
        elif kind == 'faces':
            special = make_volume(tag)[1]
            x = node_xyz(special[torch.randint(0, special.shape[0], (m,), generator=g)])
        else:
            raise KeyError(kind)
        if kind != 'faces':
            uv = O.sample_volume(x.double(), scene['tuv'].double(), scene['tbounds'].double())
            uvt = torch.cat([uv, scene['frame_dim'].double().reshape(1, 1).expand(m, 1)], -1)
            drop = tie_mask(uvt, spec)
            if kind == 'one' and drop.any():
                continue                                            # the one location sits on a tie: another location
            assert drop.float().mean() <= 0.25, (kind, n, float(drop.float().mean()))
            x = x[~drop]
        x = x[:n].contiguous()
        if x.shape[0] == n:
            return x
    raise AssertionError('no tie-free cloud: %s %d' % (kind, n))


def make_gresd(n, pattern, seed=0):
    g = torch.Generator().manual_seed(61 + seed + 7 * PATTERNS.index(pattern))
    gr = torch.randn(max(n, N_BASE), 3, generator=g)
    if pattern == 'sparse':
        gr[torch.rand(gr.shape[0], generator=g) < 0.7] = 0.0
    return gr[:n].contiguous()


def _zs(P, tag='prod'):
    """Pre-activations of the base batch (the `inside` cloud at the interior frame) in float64."""
    r = DR.deformer(make_cloud('inside', N_BASE, tag, 'tmid'), torch.zeros(N_BASE, 3), P, make_scene(tag, 'tmid'), make_spec(tag), companions=False)
    return r['z']


@functools.lru_cache(maxsize=None)
def make_params(wtag, tag='prod'):
    """Seeded float32 parameters.  `init`: nn.Linear's own scale (params._linear: U(-1/sqrt(fan_in), 1/sqrt(fan_in))).  `wide`: both
    hidden layers rescaled in turn, on the base batch and in float64, so that their pre-activations reach +-15.  `saturated-head`:
    wide, then every head row rescaled and centred so that its logit spans [-6, 6].  check_params asserts the ranges on the reference."""
    g = torch.Generator().manual_seed(71)

    def lin(o, i):
        k = 1.0 / i ** 0.5
        return (torch.rand(o, i, generator=g) * 2 - 1) * k, (torch.rand(o, generator=g) * 2 - 1) * k
    layers = [lin(32, 19), lin(32, 32), lin(3, 32)]
    dense, hsh = make_tables(tag)
    P = dict(W=[w for w, _ in layers], b=[b for _, b in layers], dense=dense, hash=hsh)
    if wtag == 'init':
        return P
    for l, name in ((0, 'z1'), (1, 'z2')):
        f = 15.0 / float(_zs(P, tag)[name].abs().max())
        P['W'][l], P['b'][l] = (P['W'][l].double() * f).float(), (P['b'][l].double() * f).float()
    if wtag == 'wide':
        return P
    assert wtag == 'saturated-head'
    z = _zs(P, tag)['z3']
    lo, hi = z.min(0).values, z.max(0).values
    f = 12.0 / (hi - lo)
    P['W'][2] = (P['W'][2].double() * f[:, None]).float()
    P['b'][2] = (P['b'][2].double() * f - f * (hi + lo) / 2.0).float()
    return P


@functools.lru_cache(maxsize=None)
def check_params(wtag, n, tag='prod'):
    """The ranges a weight set promises, asserted on the float64 reference for the first n entries of the base batch."""
    assert n <= N_BASE
    if wtag == 'init':
        return
    z = _zs(make_params(wtag, tag), tag)
    for name in ('z1', 'z2'):
        zz = z[name][:n]
        assert -15.5 <= float(zz.min()) <= -9.0 and 9.0 <= float(zz.max()) <= 15.5, (wtag, name, float(zz.min()), float(zz.max()))
    if wtag == 'saturated-head':
        zz = z['z3'][:n]
        assert -6.5 <= float(zz.min()) <= -4.5 and 4.5 <= float(zz.max()) <= 6.5, (wtag, float(zz.min()), float(zz.max()))


# ---- the fp32 oracle: torch autograd of the oracle's deformer on the CPU ------------------------------------------------------------
def oracle_sd(P, spec, dtype):
    t = lambda x: x.detach().to(dtype).clone().requires_grad_()
    sd = EC.oracle_sd(spec, P['dense'], P['hash'], dtype)
    sd = {'tpose_deformer.embedder.' + k[2:]: v for k, v in sd.items()}
    for i, k in enumerate((0, 2, 4)):
        sd['tpose_deformer.mlp.%d.weight' % k], sd['tpose_deformer.mlp.%d.bias' % k] = t(P['W'][i]), t(P['b'][i])
    return sd


def oracle_chunk(pts, g_resd, sd, scene, spec, dtype, check=True):
    """oracle.nvr_oracle.deformer's own operations in `dtype`, one by one with the intermediates kept (asserted bit-identical to it on the first 8192 entries of a case), and
    their autograd: the parameter gradients ACCUMULATE in sd's tensors; -> the per-entry matrices as plain tensors."""
    tuv, tb, fd = scene['tuv'].to(dtype), scene['tbounds'].to(dtype), scene['frame_dim'].to(dtype)
    x = pts.to(dtype)
    uv = O.sample_volume(x, tuv, tb)
    uvt = torch.cat([uv, fd.reshape(1, 1).expand(uv.shape[0], 1).to(uv.dtype)], -1)
    feat = O.hash_embed(uvt, sd, 'tpose_deformer.embedder.', spec)
    keep = [feat]
    h = feat
    for i, k in enumerate((0, 2, 4)):
        z = F.linear(h, sd['tpose_deformer.mlp.%d.weight' % k], sd['tpose_deformer.mlp.%d.bias' % k])
        keep.append(z)
        h = O.softplus(z) if i < 2 else z
        if i < 2:
            keep.append(h)
    resd = 0.05 * torch.tanh(h)
    if check:
        with torch.no_grad():
            assert torch.equal(resd, O.deformer(x, sd, spec, tuv, tb, fd))
    for t in keep:
        t.retain_grad()
    resd.backward(g_resd.to(dtype))
    feat, z1, h1, z2, h2, z3 = keep
    d = lambda t: t.detach()
    return dict(resd=d(resd), uvt=d(uvt), a0=d(feat), a1=d(h1), a2=d(h2), gz1=z1.grad, gz2=z2.grad, gz3=z3.grad, gfeat=feat.grad)


def oracle_param_grads(sd, spec):
    zero = lambda k: torch.zeros_like(sd[k]) if sd[k].grad is None else sd[k].grad
    out = {'g_dense': zero('tpose_deformer.embedder.dense'), 'g_hash': zero('tpose_deformer.embedder.hash')}
    for i, k in enumerate((0, 2, 4)):
        out['dW%d' % i], out['db%d' % i] = zero('tpose_deformer.mlp.%d.weight' % k), zero('tpose_deformer.mlp.%d.bias' % k)
    return out


def oracle(pts, g_resd, P, scene, spec, dtype=torch.float32, chunk=8192):
    """-> (per-entry dict, parameter-gradient dict) of the autograd in `dtype`, chunks of `chunk` entries."""
    sd = oracle_sd(P, spec, dtype)
    parts = [oracle_chunk(pts[i:i + chunk], g_resd[i:i + chunk], sd, scene, spec, dtype) for i in range(0, pts.shape[0], chunk)]
    ent = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]} if parts else {}
    return ent, oracle_param_grads(sd, spec)


# ---- reference + noise ----------------------------------------------------------------------------------------------------------------
def _add_refs(acc, r):
    for k in DR.PARAM_KEYS:
        acc[k] = r[k] if k not in acc else Ref(acc[k].exact + r[k].exact, acc[k].A + r[k].A, acc[k].c + r[k].c)


# the four sign patterns of three coordinates that differ by more than a global sign
_PATTERNS = torch.tensor([[1.0, 1.0, 1.0], [1.0, 1.0, -1.0], [1.0, -1.0, 1.0], [-1.0, 1.0, 1.0]], dtype=torch.float64)


def reference(pts, g_resd, P, scene, spec, trials=4, seed=0, on_chunk=None, chunk=CHUNK):
    """-> (entries, params).  params = (ref, noise, o32, touched) dicts over DR.PARAM_KEYS.  entries = list of (slice, ref, noise, o32)
    dicts over DR.ENTRY_KEYS + ('resd',), one per chunk — or, with on_chunk, nothing: on_chunk(slice, ref, noise, o32) is called per
    chunk and the chunk forgotten (the largest cases)."""
    n = pts.shape[0]
    assert trials == 4
    g = torch.Generator().manual_seed(3000 + seed)
    sign = lambda *s: torch.randint(0, 2, s, generator=g).double() * 2.0 - 1.0
    sd32 = oracle_sd(P, spec, torch.float32)
    ekeys = DR.ENTRY_KEYS + ('resd',)
    acc, pert, entries = {}, [dict() for _ in range(2 * trials)], []
    for lo in range(0, max(n, 1), chunk):
        sl = slice(lo, min(lo + chunk, n))
        x, gr = pts[sl], g_resd[sl]
        m = x.shape[0]
        r = DR.deformer(x, gr, P, scene, spec)
        _add_refs(acc, r)
        o32 = {k: [] for k in ekeys}
        for i in range(0, m, 8192):
            o = oracle_chunk(x[i:i + 8192], gr[i:i + 8192], sd32, scene, spec, torch.float32, check=lo + i == 0)
            for k in ekeys:
                o32[k].append(o[k])
        o32 = {k: torch.cat(v, 0) if v else torch.zeros_like(r[k].exact, dtype=torch.float32) for k, v in o32.items()}
        noise = {k: (o32[k].double() - r[k].exact).abs() for k in ekeys}
        x64, g64 = x.double(), gr.double()
        order = torch.rand(m, 4, generator=g).argsort(1)
        for t in range(2 * trials):
            if t < trials:                                                                                       # (b)
                sx = _PATTERNS[order[:, t]] * sign(m, 1)
                p = DR.deformer(x64 + sx * (x64.abs() + 1.0) * 2.0 ** -23, g64 + sign(m, 3) * g64.abs() * 2.0 ** -23, P, scene, spec,
                                companions=False)
            else:                                                                                                # (c)
                p = DR.deformer(x64, g64, P, scene, spec, companions=False, softplus_sign=dict(h1=sign(m, 32), h2=sign(m, 32)),
                                geometry=r['geometry'])
            for k in ekeys:
                noise[k] = torch.maximum(noise[k], (p[k].exact - r[k].exact).abs())
            for k in DR.PARAM_KEYS:
                pert[t][k] = p[k].exact if k not in pert[t] else pert[t][k] + p[k].exact
        item = (sl, {k: r[k] for k in ekeys}, noise, o32)
        if on_chunk is not None:
            on_chunk(*item)
        else:
            entries.append(item)
    for k in ('g_dense', 'g_hash'):
        acc[k] = DR.chain_c(acc[k])
    po32 = oracle_param_grads(sd32, spec)
    pnoise = {k: (po32[k].double() - acc[k].exact).abs() for k in DR.PARAM_KEYS}
    touched = {k: (acc[k].A != 0) | (po32[k] != 0) for k in ('g_dense', 'g_hash')}
    for t in range(2 * trials):
        for k in DR.PARAM_KEYS:
            pnoise[k] = torch.maximum(pnoise[k], (pert[t][k] - acc[k].exact).abs())
        for k in touched:
            touched[k] |= pert[t][k] != 0
    return entries, (acc, pnoise, po32, touched)


def reference_fwd(pts, P, scene, spec, seed=0, chunk=CHUNK):
    """reference() for the forward alone: the `resd` entry of reference(pts, zeros, P, scene, spec, seed=seed) — the same float64
    statements (DR.deformer without its backward), the same fp32 oracle (O.deformer itself, which oracle_chunk asserts its restatement
    against) and the same draws of the noise classes (b) and (c) in the same order (tests/test_deform_reference_cpu.py holds the
    two against each other bit for bit) — without the backward, the table scatters and the autograd.
    -> list of (slice, Ref, noise, o32, z) per chunk, z = the float64 pre-activations {'z1', 'z2', 'z3'} of the chunk."""
    n = pts.shape[0]
    g = torch.Generator().manual_seed(3000 + seed)
    sign = lambda *s: torch.randint(0, 2, s, generator=g).double() * 2.0 - 1.0
    sd32 = {k: v.detach() for k, v in oracle_sd(P, spec, torch.float32).items()}
    s32 = {k: scene[k].float() for k in ('tuv', 'tbounds', 'frame_dim')}
    s64 = {k: scene[k].double() for k in ('tuv', 'tbounds', 'frame_dim')}           # (converted once, not per evaluation: large volumes)
    zeros = torch.zeros(0, 3)
    out = []
    for lo in range(0, max(n, 1), chunk):
        sl = slice(lo, min(lo + chunk, n))
        x = pts[sl]
        m = x.shape[0]
        r = DR.deformer(x, zeros, P, s64, spec, backward=False)
        with torch.no_grad():
            o32 = torch.cat([O.deformer(x[i:i + 8192].float(), sd32, spec, s32['tuv'], s32['tbounds'], s32['frame_dim'])
                             for i in range(0, m, 8192)], 0) if m else torch.zeros(0, 3)
        noise = (o32.double() - r['resd'].exact).abs()
        x64 = x.double()
        order = torch.rand(m, 4, generator=g).argsort(1)
        for t in range(8):
            if t < 4:                                                                                            # (b)
                sx = _PATTERNS[order[:, t]] * sign(m, 1)
                sign(m, 3)                                                                                       # (g_resd's draw)
                p = DR.deformer(x64 + sx * (x64.abs() + 1.0) * 2.0 ** -23, zeros, P, s64, spec, companions=False, backward=False)
            else:                                                                                                # (c)
                p = DR.deformer(x64, zeros, P, s64, spec, companions=False, softplus_sign=dict(h1=sign(m, 32), h2=sign(m, 32)),
                                geometry=r['geometry'], backward=False)
            noise = torch.maximum(noise, (p['resd'].exact - r['resd'].exact).abs())
        out.append((sl, r['resd'], noise, o32, r['z']))
    return out


def accept(tag, name, val, ref, noise, o32=None, touched=None, prefix='DFB'):
    """EC.accept, unchanged: the rule, the NaN / shape checks, the exact zeros, and the K_kernel / K_oracle32 line (prefix DFB; DFF for
    the forward tests)."""
    return EC.accept(tag, name, val, ref, noise, o32, touched, report=lambda s: print(prefix + ' ' + s[4:]))


preloaded = MC.preloaded
