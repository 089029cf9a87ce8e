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
CLOUDS = ('uniform', 'far', 'inside', 'rays', 'one', 'faces')


def make_spec(tag):
    return O.embedder_geometry(bbox=BBOX, **SPECS[tag])


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
    alone and before anything runs; at most 1 % of a generated cloud may go that way."""
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
        assert drop.float().mean() <= 0.01, (kind, n, float(drop.float().mean()))
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


def accept(tag, name, val, ref, noise, o32=None, touched=None, report=print):
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
    report('ENCB %-44s %-8s K_kernel %.3g K_oracle32 %.3g max|exact| %.3g' % (tag, name, K, K32, float(ref.exact.abs().max()) if val.numel() else 0.0))
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
