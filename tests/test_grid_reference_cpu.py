"""CPU: the float64 reference of the encoder backward (tests/grid_reference.py) against float64 autograd of the oracle's
hash_embed, for every spec family and point cloud the GPU tests use.  Elementwise
    |exact - autograd| <= 16 n 2^-53 A
for the table gradients (the worst-case bound of two float64 summations of at most 8 n terms; A = the absolute-sum companion: a
cloud three box-widths wide cancels down to 1e-9 of the tensor's maximum, so the comparison is against A, not the maximum), and
A == 0 exactly where autograd's gradient is an untouched zero.  An element of g_xyz is a sum of c = 8 L F + L + 8 terms whatever n
is, each formed with at most four roundings, so its bound is max(16 n, 2 (c + 4)) 2^-53 A (two summations of c terms).  Checker
against checker: the product is not involved.

The forward reference (GR.encoder_fwd) is held to the oracle's float64 forward in the same way, its fp32 cell decision
(GR.fp32_cells) to the float64 one on tie-free clouds, and — on the `ties` cloud, where the two differ on purpose — to the oracle's
own fp32 output."""
import pytest
import torch

from tests import encoder_cases as EC
from tests import grid_reference as GR

CASES = [(tag, EC.CLOUDS[i % len(EC.CLOUDS)], 1000) for i, tag in enumerate(EC.SPECS)]
CASES += [('part-small', c, 3000) for c in EC.CLOUDS] + [('deformer-small', c, 3000) for c in EC.CLOUDS]
CASES += [('part-small', 'uniform', 20000), ('allhash', 'far', 20000), ('part-onetable', 'faces', 2000), ('part-small', 'uniform', 1)]


@pytest.mark.parametrize('tag,cloud,n', CASES, ids=['%s-%s-%d' % c for c in CASES])
def test_reference_vs_float64_autograd(tag, cloud, n):
    spec = EC.make_spec(tag)
    dense, hsh = EC.make_tables(tag)
    x = EC.make_cloud(cloud, n, spec, seed=1)
    go = EC.make_gout(n, spec, seed=1)
    ref = GR.encoder_bwd(x, go, dense, hsh, spec['bbox'], spec)
    auto = dict(zip(('g_xyz', 'g_dense', 'g_hash'), EC.oracle_bwd(x, go, dense, hsh, spec, torch.float64)))
    assert (ref['g_dense'] is None) == (not spec['separate_dense'])
    for k, r in ref.items():
        if r is None:
            continue
        assert tuple(r.exact.shape) == tuple(auto[k].shape), k
        terms = max(16 * n, 2 * (r.c + 4)) if k == 'g_xyz' else 16 * n
        err = (r.exact - auto[k]).abs()
        bound = terms * 2.0 ** -53 * r.A
        assert (err <= bound).all(), (k, float((err / bound.clamp(min=1e-300)).max()))
        rel = float((err / r.A.clamp(min=1e-300)).max())
        print('GRIDREF %-28s %-8s max |exact - autograd| / A %.3g' % ('%s-%s-%d' % (tag, cloud, n), k, rel))
        if k != 'g_xyz':
            assert ((r.A == 0) == (auto[k] == 0)).all(), k
            assert ((r.c == 0) == (r.A == 0)).all() or cloud == 'faces', k       # (a zero-weight neighbour is a summand of weight 0)
            assert (r.exact[r.A == 0] == 0).all(), k
        else:
            assert r.c == 8 * spec['L'] * spec['F'] + spec['L'] + 8
            assert (r.A >= r.exact.abs() * (1 - 1e-12)).all()


def test_tie_mask_flags_cell_boundaries():
    spec = EC.make_spec('part-small')
    b = spec['bbox'].double()
    xn = torch.tensor([[0.5, 0.3123, 0.7391], [0.31, 0.27, 0.113], [0.0, 0.27, 0.113], [1.0, 0.27, 0.113]], dtype=torch.float64)
    x = (b[0] + xn * (b[1] - b[0])).float()
    x[2, 0], x[3, 0] = spec['bbox'][0, 0], spec['bbox'][1, 0]
    m = GR.tie_mask(x, spec['bbox'], spec)
    assert m.tolist() == [True, False, True, True]          # 0.5 is a node of the res-3 level; the faces are nodes of every level
    assert GR.tie_mask(x, spec['bbox'], spec, exempt_faces=True).tolist() == [True, False, False, False]


# ---- forward ----------------------------------------------------------------------------------------------------------------------
FWD_TAGS = list(EC.SPECS) + [t for t in EC.SPECS_FWD if t not in EC.BIG_TABLES]
TIE_FREE = [c for c in EC.CLOUDS if c != 'faces']
FWD_CASES = [(tag, TIE_FREE[i % len(TIE_FREE)], 1000) for i, tag in enumerate(FWD_TAGS)]
FWD_CASES += [('part-small', c, 2000) for c in TIE_FREE] + [('deformer-small', c, 2000) for c in TIE_FREE] + [('allhash', 'far', 3000)]
TIE_TAGS = [t for t in FWD_TAGS if t.startswith('part-') and 'noinput' not in t]


@pytest.mark.parametrize('tag,cloud,n', FWD_CASES, ids=['%s-%s-%d' % c for c in FWD_CASES])
def test_forward_reference_vs_float64_oracle(tag, cloud, n):
    """|exact - hash_embed in float64| <= 2 (c + 4) 2^-53 A per element (two float64 summations of c terms, each term formed with at
    most four roundings), and the reference's fp32 cell decision IS the float64 one on a tie-free cloud."""
    spec = EC.make_spec(tag)
    dense, hsh = EC.make_tables(tag)
    x = EC.make_cloud(cloud, n, spec, seed=2)
    ref = GR.encoder_fwd(x, dense, hsh, spec['bbox'], spec)
    o64 = EC.oracle_fwd(x, dense, hsh, spec, torch.float64)
    assert tuple(ref.exact.shape) == tuple(o64.shape) == (n, spec['out_dim']) and tuple(ref.c.shape) == (spec['out_dim'],)
    err, bound = (ref.exact - o64).abs(), 2.0 * (ref.c + 4.0) * 2.0 ** -53 * ref.A
    assert (err <= bound).all(), float((err / bound.clamp(min=1e-300)).max())
    assert (ref.A >= ref.exact.abs() * (1 - 1e-12)).all()
    off = 3 if spec['include_input'] else 0
    per = 8 * spec['F'] if spec['sum'] and spec['sum_over_features'] else (8 * spec['L'] if spec['sum'] else 8)
    assert ref.c.tolist() == [1.0] * off + [float(per)] * (spec['out_dim'] - off)
    xn = GR.normalise(x, spec['bbox'])
    for l, (c0, c1) in enumerate(GR.fp32_cells(x, spec['bbox'], spec)):
        d0, d1, _ = GR.level_cells(xn, spec, l)
        assert torch.equal(c0, d0) and torch.equal(c1, d1), (tag, cloud, l)
    held = GR.encoder_fwd(x, dense, hsh, spec['bbox'], spec, cells=GR.fp32_cells(x, spec['bbox'], spec))
    assert torch.equal(held.exact, ref.exact) and torch.equal(held.A, ref.A)


@pytest.mark.parametrize('tag', TIE_TAGS)
def test_forward_reference_at_ties_holds_the_fp32_oracle(tag):
    """The `ties` cloud: the fp32 oracle's own output lies inside the acceptance rule of encoder_fwd(cells=fp32_cells) with the
    perturbation noise alone (the oracle's deviation is what is being judged, so it is not part of its own noise) — the reference is
    validated at ties, c1 - c0 == 2 included, by the oracle alone.  With the float64 cells it does NOT: the test sees the difference."""
    spec = EC.make_spec(tag)
    dense, hsh = EC.make_tables(tag)
    x = EC.make_cloud('ties', 1000, spec)
    cells = GR.fp32_cells(x, spec['bbox'], spec)
    two = torch.stack([(c1 - c0 == 2).any(1) for c0, c1 in cells]).any(0)
    assert int(two.sum()) >= 4 * 16
    ref = GR.encoder_fwd(x, dense, hsh, spec['bbox'], spec, cells=cells)
    noise, o32 = EC.forward_noise(x, dense, hsh, spec, ref, cells, with_oracle=False)
    K = EC.accept('%s-ties-1000' % tag, 'oracle32', o32, ref, noise)
    f64 = GR.encoder_fwd(x, dense, hsh, spec['bbox'], spec)
    allow = 8.0 * noise + (ref.c + 4.0) * 2.0 ** -24 * f64.A
    assert ((o32.double() - f64.exact).abs() > allow)[two].any(), 'the float64 cells would have passed too: the cloud holds no effective tie'
