"""CPU: the hand-written float64 reference of the deformer and its backward (tests/deform_reference.py) against torch's float64
autograd of oracle.nvr_oracle.deformer — so that the reference's correctness does not rest on any kernel — and the properties of the
case generators of tests/deform_cases.py that the GPU tests lean on."""
import pytest
import torch

from tests import deform_cases as DC
from tests import deform_reference as DR


@pytest.mark.parametrize('tag', ['prod', 'fallback'])
@pytest.mark.parametrize('wtag', DC.WEIGHT_SETS)
def test_reference_agrees_with_float64_autograd(wtag, tag):
    n = 300
    spec = DC.make_spec(tag)
    P = DC.make_params(wtag, tag)
    for cloud, frame, pattern in (('inside', 'tmid', 'dense'), ('faces' if tag == 'prod' else 'nodes', 't1', 'sparse'), ('outside', 't0', 'dense')):
        pts, g = DC.make_cloud(cloud, n, tag, frame), DC.make_gresd(n, pattern)
        scene = DC.make_scene(tag, frame)
        ref = DR.deformer(pts, g, P, scene, spec)
        ent, par = DC.oracle(pts, g, P, scene, spec, torch.float64)
        o64 = dict(ent, **par)
        assert set(DR.ENTRY_KEYS + DR.PARAM_KEYS + ('resd',)) <= set(o64)
        for k in DR.ENTRY_KEYS + DR.PARAM_KEYS + ('resd',):
            r, o = ref[k].exact, o64[k]
            assert r.shape == o.shape, k
            # init: 1e-12 relative, element by element (of the element's own scale A: an element that is a cancelling sum has no
            # relative accuracy in float64 either).  wide / saturated-head: 1e-12 of the tensor's largest A — torch forms tanh's
            # derivative as 1 - y^2, which at a logit of 6 is itself only good to 1e-11 of the factor; the z-based factors here are not
            scale = ref[k].A if wtag == 'init' else ref[k].A.max()
            assert ((r - o).abs() <= 1e-12 * scale + 1e-300).all(), (wtag, tag, cloud, k, float(((r - o).abs() / (scale + 1e-300)).max()))
            assert (ref[k].A >= r.abs() * (1 - 1e-12)).all(), k


def test_companions_off_and_chunks_give_the_same_values():
    spec, P, scene = DC.make_spec('prod'), DC.make_params('wide'), DC.make_scene('prod', 'tmid')
    pts, g = DC.make_cloud('inside', 100), DC.make_gresd(100, 'dense')
    a, b = DR.deformer(pts, g, P, scene, spec), DR.deformer(pts, g, P, scene, spec, companions=False)
    for k in DR.ENTRY_KEYS + DR.PARAM_KEYS:
        assert torch.equal(a[k].exact, b[k].exact) and b[k].A is None
    (e1,), p1 = DC.reference(pts, g, P, scene, spec)
    e2, p2 = DC.reference(pts, g, P, scene, spec, chunk=37)
    assert len(e2) == 3
    for k in DR.PARAM_KEYS:                                       # the parameter gradients add up over the chunks
        assert torch.allclose(p1[0][k].exact, p2[0][k].exact, rtol=0, atol=1e-13 * float(p1[0][k].A.max()))
        assert torch.equal(p1[0][k].c, p2[0][k].c) if torch.is_tensor(p1[0][k].c) else p1[0][k].c == p2[0][k].c == 100.0
    for k in DR.ENTRY_KEYS:
        cat = torch.cat([e[1][k].exact for e in e2], 0)              # (per entry independent; a matrix product may round differently per batch)
        assert ((e1[1][k].exact - cat).abs() <= 1e-13 * e1[1][k].A).all(), k


@pytest.mark.parametrize('wtag,cloud,frame', [('wide', 'inside', 'tmid'), ('saturated-head', 'nodes', 't1'), ('init', 'outside', 't0')])
def test_forward_only_reference_is_the_full_reference(wtag, cloud, frame):
    """DC.reference_fwd (the forward tests' reference) against the `resd` entry of DC.reference with a zero upstream gradient: exact, A,
    c, the fp32 oracle and the noise bit for bit, in one chunk and in three."""
    n = 100
    spec, P, scene = DC.make_spec('prod'), DC.make_params(wtag), DC.make_scene('prod', frame)
    pts = DC.make_cloud(cloud, n, 'prod', frame)
    for chunk in (DC.CHUNK, 37):
        full, _ = DC.reference(pts, torch.zeros(n, 3), P, scene, spec, chunk=chunk)
        fwd = DC.reference_fwd(pts, P, scene, spec, chunk=chunk)
        assert len(full) == len(fwd) == (1 if chunk > n else 3)
        for (sl, ref, noise, o32), (sl2, r2, n2, o2, z) in zip(full, fwd):
            assert sl == sl2 and ref['resd'].c == r2.c == 35.0
            assert torch.equal(ref['resd'].exact, r2.exact) and torch.equal(ref['resd'].A, r2.A)
            assert torch.equal(o32['resd'], o2) and torch.equal(noise['resd'], n2)
            assert set(z) == {'z1', 'z2', 'z3'} and z['z3'].shape == (sl.stop - sl.start, 3)
            assert torch.equal(r2.exact, 0.05 * torch.tanh(z['z3']))
    assert DC.reference_fwd(torch.zeros(0, 3), P, scene, spec)[0][1].exact.shape == (0, 3)


def test_weight_sets_reach_their_ranges():
    for wtag in ('wide', 'saturated-head'):
        for n in (1000, DC.N_BASE):
            DC.check_params(wtag, n)
        DC.check_params(wtag, DC.N_BASE, 'fallback')
    z = DC._zs(DC.make_params('saturated-head'))['z3']
    assert float((1.0 / torch.cosh(z) ** 2).min()) < 1e-4          # 1 - tanh^2 is a cancellation there


def test_clouds_frames_and_patterns():
    spec = DC.make_spec('prod')
    tuv, special = DC.make_volume('prod')
    assert tuple(tuv.shape) == DC.TUV_DIMS + (2,) and len(set(DC.TUV_DIMS)) == 3
    b = torch.tensor(DC.TBOUNDS)
    x = DC.make_cloud('inside', 1000)
    assert ((x >= b[0]) & (x <= b[1])).all() and torch.equal(DC.make_cloud('inside', 17), x[:17])
    x = DC.make_cloud('outside', 1000)
    assert ((x < b[0]) | (x > b[1])).all()                          # beyond the bounds on every axis
    x = DC.make_cloud('one', 1000)
    assert (x == x[:1]).all()
    # `nodes` and `faces` sit exactly on voxel nodes: the sampled (u, v) IS the node's value, in fp32 and in float64
    from oracle import nvr_oracle as O
    for kind in ('nodes', 'faces'):
        x = DC.make_cloud(kind, 1000)
        idx = (x.double() - b[0].double()) / (b[1] - b[0]).double() * (torch.tensor(DC.TUV_DIMS).double() - 1.0)
        assert torch.equal(idx, idx.round())
        want = tuv[idx[:, 0].long(), idx[:, 1].long(), idx[:, 2].long()]
        assert torch.equal(O.sample_volume(x, tuv, b), want)
        assert torch.equal(O.sample_volume(x.double(), tuv.double(), b.double()), want.double())
    uv = O.sample_volume(DC.make_cloud('faces', 1000), tuv, b)
    assert ((uv == 0.0) | (uv == 1.0)).any()
    q = uv[:, :1].double() / spec['size'].double()[None]             # u on a level-cell boundary (to fp32 rounding of k * cell)
    assert (((q - q.round()).abs() < 1e-6) & (q.round() >= 1)).any(1).float().mean() > 0.3
    # normalised t: 0, interior, 1
    assert [DC.FRAMES[k] for k in ('t0', 'tmid', 't1')] == [0.0, 0.37, 1.0] and DC.BBOX[0][2] == 0.0 and DC.BBOX[1][2] == 1.0
    g = DC.make_gresd(1000, 'sparse')
    assert 0.6 < float((~g.any(1)).float().mean()) < 0.8 and DC.make_gresd(1000, 'dense').all()


@pytest.mark.parametrize('wtag', DC.WEIGHT_SETS)
def test_fp32_oracle_is_inside_the_rule(wtag):
    """The cases are well conditioned: torch's own fp32 evaluation passes the rule on every output, and a sparse upstream gradient
    leaves exactly zero gradient rows."""
    n = 1000
    spec, P = DC.make_spec('prod'), DC.make_params(wtag)
    for cloud, frame, pattern in (('inside', 'tmid', 'dense'), ('faces', 't1', 'sparse'), ('one', 't0', 'sparse')):
        pts, g = DC.make_cloud(cloud, n), DC.make_gresd(n, pattern)
        ((_, ref, noise, o32),), (pref, pnoise, po32, touched) = DC.reference(pts, g, P, DC.make_scene('prod', frame), spec)
        cid = '%s-%s-%s-%s' % (wtag, cloud, frame, pattern)
        for k in DR.ENTRY_KEYS:
            DC.accept(cid, k, o32[k], ref[k], noise[k], o32[k])
        for k in DR.PARAM_KEYS:
            DC.accept(cid, k, po32[k], pref[k], pnoise[k], po32[k], touched.get(k) if cloud == 'faces' else None)
        if pattern == 'sparse':
            zero = ~g.any(1)
            for k in ('gz1', 'gz2', 'gz3', 'gfeat'):
                assert not ref[k].A[zero].any(), k
