"""CPU: the hand-written float64 reference of the part MLPs and their backward (tests/mlp_reference.py) against torch's float64
autograd of invr.autograd.part_mlps_torch — so that the reference's correctness does not rest on any kernel — and the properties of
the case generators of tests/mlp_cases.py that the GPU tests lean on."""
import pytest
import torch

from tests import mlp_cases as MC
from tests import mlp_reference as MR


@pytest.mark.parametrize('n_rgb', [2, 3])
@pytest.mark.parametrize('tag', MC.WEIGHT_SETS)
def test_reference_agrees_with_float64_autograd(tag, n_rgb):
    n = 300
    emb, dirs = MC.make_inputs(n)
    P = MC.with_latent(MC.make_params(tag, n_rgb), MC.NUM_LATENT - 1)
    for pattern in ('dense', 'sparse'):
        g_raw = MC.make_graw(n, pattern)
        ref = MC.flatten(MR.part_mlps(emb, dirs, P, g_raw))
        o64 = MC.flatten(MC.oracle(emb, dirs, P, g_raw, torch.float64))
        assert set(ref) == set(o64) and len(ref) == (23 if n_rgb == 3 else 19)
        for k in ref:
            r, o = ref[k].exact, o64[k]
            assert r.shape == o.shape, k
            # init: 1e-12 relative, element by element (of the element's own scale A: an element that is a cancelling sum has no
            # relative accuracy in float64 either).  wide / dead: 1e-12 of the tensor's largest A — torch forms the sigmoid's derivative
            # as s (1 - s), which at a logit of 20 is itself only good to 5e-8 of the factor; the z-based factors here are not
            scale = ref[k].A if tag == 'init' else ref[k].A.max()
            assert ((r - o).abs() <= 1e-12 * scale + 1e-300).all(), (tag, n_rgb, pattern, k, float(((r - o).abs() / (scale + 1e-300)).max()))
            assert (ref[k].A >= r.abs() * (1 - 1e-12)).all(), k


def test_companions_off_gives_the_same_values():
    emb, dirs = MC.make_inputs(50)
    P = MC.with_latent(MC.make_params('wide', 3), 0)
    g = MC.make_graw(50, 'dense')
    a, b = MC.flatten(MR.part_mlps(emb, dirs, P, g)), MC.flatten(MR.part_mlps(emb, dirs, P, g, companions=False))
    for k in a:
        assert torch.equal(a[k].exact, b[k].exact) and b[k].A is None


def test_slot_order_round_trip():
    x = torch.arange(70, dtype=torch.float64)[None] + 1.0
    s = MR.slot_a2(x)
    assert s.shape == (1, 72) and (s[0, MR.PAD_SLOTS] == 0).all() and MR.PAD_SLOTS == [19, 55]
    assert torch.equal(MR.unslot_a2(s), x)
    from invr import autograd as AG                               # the product's own copy of the map
    assert [AG._rgb1_col(j >> 2, j & 3) for j in range(72)] == MR.SLOT_COL


@pytest.mark.parametrize('n_rgb', [2, 3])
def test_weight_sets_reach_their_ranges(n_rgb):
    for tag in ('wide', 'dead'):
        for n in (1000, 5000):
            MC.check_params(tag, n_rgb, n)
    z = MC._zs(MC.make_params('dead', n_rgb))
    for name in MC.HIDDEN[n_rgb]:                                  # (the derivative factors the `dead` rows are made of)
        assert float(MR.dsoftplus(z[name][:, MC.dead_units(name)]).max()) < 2.5e-3


def test_inputs_and_patterns():
    emb, dirs = MC.make_inputs(1000)
    assert not dirs[0].any() and abs(float(dirs[1].norm()) - 12.0) < 1e-5
    nrm = dirs[2:].norm(dim=1)
    assert 0.5 <= float(nrm.min()) and float(nrm.max()) <= 1.5 + 1e-6
    assert torch.equal(MC.make_inputs(17)[0], emb[:17])
    g = MC.make_graw(1000, 'sparse')
    zero = ~g.any(1)
    assert 0.6 < float(zero.float().mean()) < 0.8
    assert not MC.make_graw(10, 'occ-only')[:, :3].any() and not MC.make_graw(10, 'rgb-only')[:, 3].any()


@pytest.mark.parametrize('n_rgb', [2, 3])
@pytest.mark.parametrize('tag', MC.WEIGHT_SETS)
def test_fp32_oracle_is_inside_the_rule(tag, n_rgb):
    """The cases are well conditioned: torch's own fp32 evaluation passes the rule on every output, and a sparse upstream gradient
    leaves exactly zero gradient rows."""
    n = 1000
    emb, dirs = MC.make_inputs(n)
    P = MC.with_latent(MC.make_params(tag, n_rgb), MC.NUM_LATENT - 1)
    for pattern in MC.PATTERNS:
        g_raw = MC.make_graw(n, pattern)
        ref, noise, o32 = MC.reference(emb, dirs, P, g_raw)
        for k in ref:
            MC.accept('%s-%d-%s' % (tag, n_rgb, pattern), k, o32[k], ref[k], noise[k], o32[k])
        if pattern == 'sparse':
            zero = ~g_raw.any(1)
            for k in ('gz0', 'gz1', 'gz2', 'gz4', 'g_emb'):
                assert not ref[k].A[zero].any(), k
