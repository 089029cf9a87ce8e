"""Test infrastructure shared by the encoder-backward tests (tests/test_grid_reference_cpu.py, tests/test_gpu_encoder_bwd.py and
its wave-machine twin): spec families, seeded tables, point clouds, the oracle's autograd as the fp32 reference, the per-element
noise scale and the acceptance rule.  Checker only — nothing of the product is imported here."""
import functools

import torch

from oracle import nvr_oracle as O
from tests import grid_reference as GR

BBOX = [[-0.5, -1.0, -0.3], [0.5, 0.9, 0.4]]            # non-cubic, off-origin
_PART = dict(n_levels=16, n_features_per_level=16, b=1.38, base_resolution=2, sum=True, sum_over_features=True, separate_dense=True)
_DEFORMER = dict(n_levels=8, n_features_per_level=2, log2_hashmap_size=14, base_resolution=4, b=1.38, sum=False,
                 sum_over_features=True, separate_dense=True, include_input=True)      # config.DEFAULTS tpose_deformer (pinned in the GPU module)
_D2 = dict(n_levels=8, n_features_per_level=2, base_resolution=4, b=1.5, sum=False, sum_over_features=True, separate_dense=True)
SPECS = {
    'part-small': dict(_PART, log2_hashmap_size=12),                      # T 4099, start_hash 7: thousands of points per hashed row
    'part-prod': dict(_PART, log2_hashmap_size=18),                       # start_hash 11: small 0-5, cached 6-10, 5 hashed
    'part-onetable': dict(_PART, log2_hashmap_size=12, separate_dense=False),
    'deformer': _DEFORMER,
    'deformer-small': dict(_D2, log2_hashmap_size=10),                    # every level slice fits the generic kernel's LDS
    'deformer-nolds': dict(_D2, log2_hashmap_size=16),                    # res 30 (54,000 floats) and T 65,537 x 2 do not
    'rowscalar-generic': dict(n_levels=8, n_features_per_level=4, log2_hashmap_size=10, base_resolution=4, b=1.5, sum=True,
                              sum_over_features=True, separate_dense=True),
    'allhash': dict(n_levels=6, n_features_per_level=4, log2_hashmap_size=8, base_resolution=8, b=1.38, sum=True,
                    sum_over_features=False, separate_dense=True),        # start_hash 0: one (L,T,F) table, sum over levels
    'part-small-noinput': dict(_PART, log2_hashmap_size=12, include_input=False),
    'deformer-small-noinput': dict(_D2, log2_hashmap_size=10, include_input=False),
}
# forward-only families (tests/test_gpu_encoder_fwd.py), beside the ones above: kept out of SPECS, whose every member the backward
# tests build full-size float64 gradient tables for
SPECS_FWD = {
    'part-base16': dict(_PART, base_resolution=16, log2_hashmap_size=16),  # level 0 = 16^3 = 4096 rows: the whole LDS stage (the body's case)
    'part-t9': dict(_PART, log2_hashmap_size=9),                          # T 521 < 1024: the fp64 modulo inside the part kernels
    'part-t19': dict(_PART, log2_hashmap_size=19),                        # T 2^19 + 21: the two-round 24-bit modulo under the x-delta fold
    'part-t20': dict(_PART, log2_hashmap_size=20),                        # T 2^20 + 7: the production constants of the one-round modulo
}
BBOX_OF = {'part-base16': [[-1, -1.2, -0.34], [0.8, 0.7, 0.5]]}           # the body's box (config.DEFAULTS); every other family: BBOX.  (In BBOX no
#                                                                           fp32 z reaches c1 - c0 == 2 on the three dense levels of this family.)
BIG_TABLES = ('part-t19', 'part-t20')                                     # 134 / 336 MB of fp32 tables: n <= 1000, never on the wave machine's default run
CLOUDS = ('uniform', 'far', 'inside', 'rays', 'one', 'faces')


def make_spec(tag):
    return O.embedder_geometry(bbox=BBOX_OF.get(tag, BBOX), **(SPECS[tag] if tag in SPECS else SPECS_FWD[tag]))


@functools.lru_cache(maxsize=2)
def make_tables(tag):
    """Seeded ~N(0, 0.1^2) tables -> (dense (dense_rows,F) or None, hash)."""
    sp = make_spec(tag)
    g = torch.Generator().manual_seed(sum(map(ord, tag)))
    dense = torch.randn(sp['dense_rows'], sp['F'], generator=g) * 0.1 if sp['separate_dense'] else None
    hsh = torch.randn(sp['n_hash'], sp['T'], sp['F'], generator=g) * 0.1
    return dense, hsh


def _raw_cloud(kind, m, g):
    """(m,3) float64 normalised coordinates."""
    u = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    if kind == 'uniform':
        return u(m, 3) * 1.2 - 0.1
    if kind == 'far':
        return u(m, 3) * 3.0 - 1.0
    if kind == 'inside':
        return u(m, 3)
    if kind == 'rays':                                      # runs of 64 consecutive samples along short segments
        runs = (m + 63) // 64
        o = u(runs, 1, 3) * 1.1 - 0.05
        d = torch.randn(runs, 1, 3, generator=g, dtype=torch.float64)
        d = d / d.norm(dim=-1, keepdim=True) * (0.05 + 0.2 * u(runs, 1, 1))
        s = torch.arange(64, dtype=torch.float64)[None, :, None] / 64.0
        return (o + d * s).reshape(-1, 3)[:m]
    if kind == 'one':
        return u(1, 3) * 0.9 + 0.05 + (u(m, 3) - 0.5) * 2e-5
    if kind == 'faces':
        return u(m, 3) * 1.2 - 0.1
    raise KeyError(kind)


def make_cloud(kind, n, spec, seed=0):
    """-> x (n,3) float32 world coordinates.  Points on cell ties (GR.tie_mask) are removed from the inputs, by the float64 reference
    alone and before anything runs; at most 1 % of a generated cloud may go that way (resolutions up to 666; more above, see below)."""
    if kind == 'ties':
        return make_ties(n, spec, seed)
    if kind == 'wrap':
        return make_wrap(n, spec, seed)
    bounds = spec['bbox']
    b = bounds.double()
    for attempt in range(8):
        g = torch.Generator().manual_seed(1000 * seed + 17 * CLOUDS.index(kind) + attempt)
        m = n + max(4096, n // 16)                        # (a generated cloud large enough for the 1 % to mean something)
        xn = _raw_cloud(kind, m, g)
        x = (b[0] + xn * (b[1] - b[0])).float()
        if kind == 'faces':                                 # fp32 coordinates EQUAL to the bounds on one, two or three axes
            k = torch.randint(1, 4, (m,), generator=g)
            axes = torch.rand(m, 3, generator=g).argsort(1)
            side = torch.randint(0, 2, (m, 3), generator=g)
            for j in range(3):
                on = k > j
                a = axes[:, j]
                val = bounds[side[:, j], a]
                x[on, a[on]] = val[on]
        drop = GR.tie_mask(x, bounds, spec, exempt_faces=kind == 'faces')
        if kind == 'one' and drop.float().mean() > 0.01:    # the one location itself sits on a tie: another location
            continue
        # (the band is 2^-20 q either side of a node: 3 axes x 2^-19 x res / 2 per level, x 3.6 for the levels below it in b = 1.38 steps
        #  = 1e-5 res of the finest level — 0.25 % at res 250, 2 % at the 2008 of a base-16 family, which gets 1.5 times that)
        cap = max(0.01, 1.5e-5 * max(spec['res']))
        assert drop.float().mean() <= cap, (kind, n, float(drop.float().mean()))
        x = x[~drop][:n].contiguous()
        assert x.shape[0] == n
        return x
    raise AssertionError('no tie-free location for the `one` cloud')


def make_gout(n, spec, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    return torch.randn(n, spec['out_dim'], generator=g)


def oracle_sd(spec, dense, hsh, dtype):
    sd = {'e.bounds': spec['bbox'].to(dtype), 'e.entries_size': spec['size'].to(dtype), 'e.entries_num': torch.tensor(spec['res']),
          'e.entries_sum': spec['entries_sum'], 'e.offsets': GR.corner_offsets().to(dtype), 'e.hash': hsh.to(dtype).clone().requires_grad_()}
    if spec['separate_dense']:
        sd['e.dense'] = dense.to(dtype).clone().requires_grad_()
    return sd


def oracle_bwd(x, g_out, dense, hsh, spec, dtype, chunk=8192):
    """Autograd of O.hash_embed in `dtype` (chunks of `chunk` points; the table gradients accumulate) -> g_xyz, g_dense, g_hash."""
    sd = oracle_sd(spec, dense, hsh, dtype)
    gx = []
    for i in range(0, x.shape[0], chunk):
        xc = x[i:i + chunk].to(dtype).clone().requires_grad_()
        out = O.hash_embed(xc, sd, 'e.', spec)
        out.backward(g_out[i:i + chunk].to(dtype))
        gx.append(xc.grad)
    zero = lambda k: torch.zeros_like(sd[k]) if sd[k].grad is None else sd[k].grad
    return (torch.cat(gx, 0) if gx else torch.zeros(0, 3, dtype=dtype)), (zero('e.dense') if spec['separate_dense'] else None), zero('e.hash')


def noise_of(x, g_out, dense, hsh, spec, ref, trials=4, seed=0):
    """The convention of tests/conditioning.py, per element of every output: the larger of (a) the deviation from `exact` of the
    oracle's own fp32 autograd (the reference's arithmetic: it rounds the normalised coordinate exactly as a kernel does) and (b) the
    largest move of `exact` under `trials` independent perturbations x + s (|x| + 1) 2^-23, s = +-1 per coordinate.
    -> (noise dict, the fp32 oracle's gradients dict, touched dict: elements that the exact, a perturbed or the fp32 evaluation reaches)."""
    keys = [k for k in ('g_xyz', 'g_dense', 'g_hash') if ref[k] is not None]
    o32 = dict(zip(('g_xyz', 'g_dense', 'g_hash'), oracle_bwd(x, g_out, dense, hsh, spec, torch.float32)))
    noise = {k: (o32[k].double() - ref[k].exact).abs() for k in keys}
    touched = {k: (ref[k].A != 0) | (o32[k] != 0) for k in keys}
    g = torch.Generator().manual_seed(3000 + seed)
    x64 = x.double()
    for _ in range(trials):
        s = torch.randint(0, 2, x64.shape, generator=g).double() * 2.0 - 1.0
        p = GR.encoder_bwd(x64 + s * (x64.abs() + 1.0) * 2.0 ** -23, g_out, dense, hsh, spec['bbox'], spec, companions=False)
        for k in keys:
            noise[k] = torch.maximum(noise[k], (p[k].exact - ref[k].exact).abs())
            touched[k] |= p[k].exact != 0
    return noise, o32, touched


def headroom(val, ref, noise):
    """K = max_e |val - exact| / (noise + 2^-23 A) over the elements with a non-zero denominator."""
    den = noise + 2.0 ** -23 * ref.A
    err = (val.double() - ref.exact).abs()
    m = den > 0
    return float((err[m] / den[m]).max()) if m.any() else 0.0


def accept(tag, name, val, ref, noise, o32=None, touched=None, report=print, prefix='ENCB'):
    """The acceptance rule, every element, none left out:
        |kernel - exact| <= 8 noise + (c + 4) 2^-24 A + c 2^-126
    (c + 4) 2^-24 A is the rigorous bound of an fp32 sum of c terms in ANY order, each term formed with at most four roundings;
    c 2^-126 covers float atomics that flush denormals.  A == 0 (a row no point touches) requires exactly 0.0; with `touched` (the
    `faces` cloud) only where no evaluation reaches the element."""
    assert tuple(val.shape) == tuple(ref.exact.shape), (name, val.shape, ref.exact.shape)
    assert not torch.isnan(val).any(), '%s %s: %d elements not written / NaN' % (tag, name, int(torch.isnan(val).sum()))
    c = ref.c if torch.is_tensor(ref.c) else float(ref.c)
    allow = 8.0 * noise + (c + 4.0) * 2.0 ** -24 * ref.A + c * 2.0 ** -126
    err = (val.double() - ref.exact).abs()
    K = headroom(val, ref, noise)
    K32 = headroom(o32, ref, noise) if o32 is not None else float('nan')
    report(prefix + ' %-44s %-8s K_kernel %.3g K_oracle32 %.3g max|exact| %.3g' % (tag, name, K, K32, float(ref.exact.abs().max()) if val.numel() else 0.0))
    bad = err > allow
    if bad.any():
        i = int((err - allow).argmax())
        raise AssertionError('%s %s: %d of %d elements outside the rule; worst flat index %d: kernel %.9g exact %.9g allowed %.3g noise %.3g A %.3g'
                             % (tag, name, int(bad.sum()), bad.numel(), i, float(val.reshape(-1)[i]), float(ref.exact.reshape(-1)[i]),
                                float(allow.reshape(-1)[i]), float(noise.reshape(-1)[i]), float(ref.A.reshape(-1)[i])))
    zero = ref.A == 0
    if touched is not None:
        zero = zero & ~touched
    assert (val[zero] == 0.0).all(), '%s %s: %d untouched elements are not exactly 0' % (tag, name, int((val[zero] != 0).sum()))
    return K


# ---- forward ----------------------------------------------------------------------------------------------------------------------
TIE_KINDS = ('dense-z', 'hash-x', 'hash-y', 'hash-z', 'integer', 'below', 'above', 'dense-x', 'dense-y')


@functools.lru_cache(maxsize=4)
def _tie_coordinates(res, size, sh, b0, b1, seed):
    """Per TIE_KIND the fp32 coordinates (axis, value) that show the pattern at some level, found by the reference's arithmetic alone
    (GR.fp32_cells' per-axis statement): for a level, an axis and an integer k the 8193 floats around b0 + k cell ext are scanned.
        c1 - c0 == 2   f the largest float below a power-of-two k <= res - 2 (f + 1.0f rounds up): '<dense|hash>-<axis>'
        f == k, f the float below / above k (any 1 <= k <= res - 2): 'integer', 'below', 'above' — the cell decision at its edge"""
    g = torch.Generator().manual_seed(500 + seed)
    found = {k: [] for k in TIE_KINDS}
    steps = torch.arange(-4096, 4097, dtype=torch.int32)
    for l, (r, cell) in enumerate(zip(res, size)):
        cell = torch.tensor(cell, dtype=torch.float32)
        pow2 = [k for k in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024) if k <= r - 2]
        others = [int(k) for k in torch.randint(1, max(r - 1, 2), (2,), generator=g).tolist() if 1 <= k <= r - 2]
        for a in range(3):
            lo, ext = torch.tensor(b0[a], dtype=torch.float32), torch.tensor(b1[a], dtype=torch.float32) - torch.tensor(b0[a], dtype=torch.float32)
            for k in pow2 + others:
                centre = (lo.double() + k * cell.double() * ext.double()).float()
                if abs(float(centre)) < 1e-3:                   # (neighbouring bit patterns would cross zero)
                    continue
                xs = (centre.view(torch.int32) + steps).view(torch.float32)
                f = ((xs - lo) / ext) / cell                    # :112, :115 in fp32
                c0, c1 = f.long().clamp(0, r - 1), (f + 1.0).long().clamp(0, r - 1)
                kf = torch.tensor(float(k))
                if k in pow2:
                    found[('hash-' if l >= sh else 'dense-') + 'xyz'[a]] += [(a, float(v)) for v in xs[c1 - c0 == 2][:8]]
                for name, target in (('integer', kf), ('below', torch.nextafter(kf, kf - 1)), ('above', torch.nextafter(kf, kf + 1))):
                    found[name] += [(a, float(v)) for v in xs[f == target][:1]]
    return found


def make_ties(n, spec, seed=0):
    """The `ties` cloud -> x (n,3) fp32: point i carries one coordinate of kind TIE_KINDS[i % 9] (its other two coordinates uniform
    inside the box).  Asserted here, by GR.fp32_cells and before anything runs: at least min(16, n // 9) points with c1 - c0 == 2
    on the z axis of a dense level and on each of the x, y, z axes of a hashed level."""
    bounds = spec['bbox']
    found = _tie_coordinates(tuple(spec['res']), tuple(float(s) for s in spec['size']), spec['start_hash'],
                             tuple(bounds[0].tolist()), tuple(bounds[1].tolist()), seed)
    g = torch.Generator().manual_seed(9000 + seed)
    b = bounds.double()
    x = (b[0] + torch.rand(n, 3, generator=g, dtype=torch.float64) * (b[1] - b[0])).float()
    for i in range(n):
        cand = found[TIE_KINDS[i % len(TIE_KINDS)]]
        if cand:
            a, v = cand[(i // len(TIE_KINDS)) % len(cand)]
            x[i, a] = v
    cells = GR.fp32_cells(x, bounds, spec)
    sh = spec['start_hash']
    two = lambda levels, a: int(torch.stack([cells[l][1][:, a] - cells[l][0][:, a] == 2 for l in levels]).any(0).sum())
    want = min(16, n // len(TIE_KINDS))
    counts = {'dense-z': two(range(sh), 2), 'hash-x': two(range(sh, spec['L']), 0), 'hash-y': two(range(sh, spec['L']), 1),
              'hash-z': two(range(sh, spec['L']), 2)}
    assert all(v >= want for v in counts.values()), (counts, want)
    return x.contiguous()


def make_wrap(n, spec, seed=0):
    """The `wrap` cloud -> x (n,3) fp32 inside the box: points of which, at some hashed level, the two x corners of a (y, z) corner
    pair lie on either side of the table's end — the c1x row is the c0x row + a small delta folded back into [0, T), in both
    directions.  (x's hash prime is 1: without the modulo the two rows are a few apart, so rows more than T / 2 apart have wrapped.)
    One point in T / 60 or so of a uniform cloud is one; they are found by the reference's arithmetic alone (GR.fp32_cells,
    GR.level_rows) among up to 4 M uniform points.  Asserted here: at least min(n, 32) / 4 in each direction; the rest is uniform."""
    bounds, T, sh, L = spec['bbox'], spec['T'], spec['start_hash'], spec['L']
    b = bounds.double()
    g = torch.Generator().manual_seed(7000 + seed)
    up, down, plain = [], [], None
    want = max(n // 2, 1)
    for _ in range(16):
        x = (b[0] + torch.rand(262144, 3, generator=g, dtype=torch.float64) * (b[1] - b[0])).float()
        cells = GR.fp32_cells(x, bounds, spec)
        u = torch.zeros(x.shape[0], dtype=torch.bool)
        d = torch.zeros_like(u)
        for l in range(sh, L):
            rows = GR.level_rows(cells[l][0], cells[l][1], spec, l)
            for k in range(4):                                  # (rows[k]: the c0x corner, rows[k + 4]: the c1x corner of the same y, z)
                u |= rows[k] - rows[k + 4] > T // 2
                d |= rows[k + 4] - rows[k] > T // 2
        up.append(x[u]); down.append(x[d])
        plain = x[~(u | d)] if plain is None else plain
        if sum(map(len, up)) >= want and sum(map(len, down)) >= want:
            break
    up, down = torch.cat(up)[:want], torch.cat(down)[:want]
    need = min(n, 32) // 4
    assert len(up) >= need and len(down) >= need, (len(up), len(down), need)
    pick = lambda i: (up, down)[i % 2][i // 2] if i // 2 < len((up, down)[i % 2]) else plain[i]       # up, down, up, ... then uniform
    return torch.stack([pick(i) for i in range(n)]).contiguous() if n else torch.zeros(0, 3)


def oracle_fwd(x, dense, hsh, spec, dtype, chunk=65536):
    """O.hash_embed in `dtype` (the tables are converted only when `dtype` is not theirs)."""
    sd = {'e.bounds': spec['bbox'].to(dtype), 'e.entries_size': spec['size'].to(dtype), 'e.entries_num': torch.tensor(spec['res']),
          'e.entries_sum': spec['entries_sum'], 'e.offsets': GR.corner_offsets().to(dtype), 'e.hash': hsh.to(dtype)}
    if spec['separate_dense']:
        sd['e.dense'] = dense.to(dtype)
    with torch.no_grad():
        out = [O.hash_embed(x[i:i + chunk].to(dtype), sd, 'e.', spec) for i in range(0, x.shape[0], chunk)]
    return torch.cat(out, 0) if out else torch.zeros(0, spec['out_dim'], dtype=dtype)


def forward_noise(x, dense, hsh, spec, ref, cells, trials=4, seed=0, with_oracle=True):
    """noise_of's convention for the forward, per element: the larger of (a) the deviation from `exact` of O.hash_embed in fp32 and
    (b) the largest move of `exact` under `trials` perturbations x + s (|x| + 1) 2^-23, s = +-1 per coordinate, with the cells held.
    -> noise (n,out_dim), the fp32 oracle's output.  with_oracle False leaves (a) out: the rule the oracle ITSELF is held to on the
    `ties` cloud (tests/test_grid_reference_cpu.py)."""
    o32 = oracle_fwd(x, dense, hsh, spec, torch.float32)
    noise = (o32.double() - ref.exact).abs() if with_oracle else torch.zeros_like(ref.exact)
    g = torch.Generator().manual_seed(3000 + seed)
    x64 = x.double()
    for _ in range(trials):
        s = torch.randint(0, 2, x64.shape, generator=g).double() * 2.0 - 1.0
        p = GR.encoder_fwd(x64 + s * (x64.abs() + 1.0) * 2.0 ** -23, dense, hsh, spec['bbox'], spec, cells=cells, companions=False)
        noise = torch.maximum(noise, (p.exact - ref.exact).abs())
    return noise, o32
