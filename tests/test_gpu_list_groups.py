"""GPU: the multi-group walk of the per-part pair lists and winner lists (csrc/pair_lists.h, csrc/k_lists.hip) in EVERY merge mode,
against its own single-group case.

A frame with more than two groups of 4096 survivor slots exercises the group bases (sums of the gcount rows before a group), the
rank walk across tiles, the winner segments and the colour kernel's segment cursor; the same rays rendered in chunks of 256 stay
inside ONE group per call (asserted: the frame's 4670 rays hold 45 k survivors, up to 3497 per chunk; chunks of 1024 rays would hold
up to 12539, three groups).  A pair's value does not depend on its position in the lists, so the two renders must agree bit for bit —
any disagreement between the multi-group and the single-group walk shows, whether in ranks, bases, winner segments or the cursor.
The default merge is also pinned list by list in tests/test_gpu_production_kernels.py; every mode is held survivor by
survivor to the reference's merge in tests/test_gpu_merge_modes.py. tests/test_hostsim_list_groups_cpu.py runs the same body through the host build."""
import copy

import pytest
import torch

import tests.test_gpu_production_kernels as P
from invr import scene

RES, S, POSE, CHUNK, GROUP = 96, 64, 2, 256, 4096
AGGRS = ['', 'mean', 'dist', 'mindist']


def make_small_net(dev, n_samples=S):
    """The reduced model of the host-build tests (2^12-row tables; also tests/test_hostsim_production_cpu.py), on `dev`."""
    from invr.config import make_cfg
    from invr.network import Network
    torch.manual_seed(11)
    cfg = make_cfg(table_log2=12, N_samples=n_samples)
    net = Network(cfg=copy.deepcopy(cfg)).eval()
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith('embedder.dense') or name.endswith('embedder.hash'):
                p.normal_(0.0, 0.1, generator=g)
    return cfg, net.to(dev)


def check_list_groups(cfg0, net, aggr, dev):
    """The frame of tests/test_gpu_production_kernels.make_frame (pose 2, 96 x 96 pixels x 64 samples) with cfg.aggr = aggr: whole
    against chunks of CHUNK rays."""
    kw = dict(P.POSES[POSE])
    thresh = kw.pop('thresh')
    bnp, _ = scene.make_scene(RES, RES, **kw)
    gb = {k: v.to(dev) for k, v in scene.to_torch(bnp).items()}
    cfg = copy.deepcopy(cfg0)
    cfg.smpl_thresh = thresh
    cfg.aggr = aggr
    old = net.cfg
    net.cfg = cfg
    try:
        ctx = net.prepare(gb)
        ro, rd, nr, fa = (gb[k][0] for k in ('ray_o', 'ray_d', 'near', 'far'))

        def render(r0, r1):
            o = net.render_rays(ctx, ro[r0:r1], rd[r0:r1], nr[r0:r1], fa[r0:r1], S, want_raw=True)
            return {k: o[k].cpu().clone() for k in ('rgb_map', 'acc_map', 'raw', 'stats')}

        n = ro.shape[0]
        whole = render(0, n)
        while int(whole['stats'][0]) % 8 == 0 and n > ro.shape[0] - 64:          # the ragged flag-byte tail must be exercised
            n -= 1
            whole = render(0, n)
        na = int(whole['stats'][0])
        print('aggr %r: %d rays, %d survivors (%d groups)' % (aggr, n, na, (na - 1) // GROUP + 1))
        assert na > 2 * GROUP, na
        assert na % 8 != 0, na
        assert int(whole['stats'][6]) == 0
        parts = [render(r0, min(r0 + CHUNK, n)) for r0 in range(0, n, CHUNK)]
    finally:
        net.cfg = old
    nas = [int(p['stats'][0]) for p in parts]
    print('survivors per chunk:', nas)
    assert all(x <= GROUP for x in nas), nas
    assert sum(x > 0 for x in nas) * 2 >= len(nas), nas
    assert all(int(p['stats'][6]) == 0 for p in parts)
    assert sum(nas) == na, (sum(nas), na)
    for k in ('rgb_map', 'acc_map', 'raw'):
        assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), (aggr, k)


@pytest.fixture(scope='module')
def small_net():
    return make_small_net('cuda:0')


@pytest.mark.gpu
@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_list_groups_whole_frame_equals_single_group_chunks(small_net, aggr):
    check_list_groups(*small_net, aggr, 'cuda:0')
