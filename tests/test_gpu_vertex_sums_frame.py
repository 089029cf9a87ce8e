"""GPU: a whole eval frame with the de-hashed vertex tables (cfg.eval_vertex_rows) against the same frame without them — rgb_map,
acc_map and raw bit for bit — and the tables' cache: after an in-place change of a part's hash table + invalidate_row_sums() the
render is that of a fresh network holding the changed table (a stale vertex table would show the old one).
64 x 64 rays x 32 samples, make_cfg(table_log2=12): T = 4099, so the base-2 parts hash from level 7 (res 19) and the body from level
1 (res 22).  The cap 2^17 moves levels 7 .. 10 (res <= 50) of the base-2 parts and 1 .. 3 (res <= 42) of the body: some, not all,
of the hashed levels of every part."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
RES, S, CAP = 64, 32, 2 ** 17


def _cfg(rows):
    from invr.config import make_cfg
    return make_cfg(table_log2=12, N_samples=S, eval_vertex_rows=rows)


def _net(rows, sd=None):
    import invr  # noqa: F401
    from invr import params
    from invr.network import Network
    cfg = _cfg(rows)
    net = Network(cfg=cfg)
    net.load_state_dict(sd if sd is not None else params.init_state_dict(cfg, seed=4), strict=True)
    return net.to(DEV).eval()


@pytest.fixture(scope='module')
def frame():
    from invr import scene
    b, _ = scene.make_scene(RES, RES, seed=0, cam_dist=1.8, frame=3, pose_seed=0)
    b = {k: v.to(DEV) for k, v in scene.to_torch(b).items()}
    return b, tuple(b[k][0].contiguous() for k in ('ray_o', 'ray_d', 'near', 'far'))


def _render(net, frame):
    b, a = frame
    o = net.render_rays(b, a[0], a[1], a[2], a[3], S, want_raw=True)
    torch.cuda.synchronize()
    return {k: o[k].clone() for k in ('rgb_map', 'acc_map', 'raw')}


def _same(a, b, what):
    for k in ('rgb_map', 'acc_map', 'raw'):
        assert not torch.isnan(a[k]).any() and torch.equal(a[k], b[k]), '%s: %s differs in %d elements' % (what, k, int((a[k] != b[k]).sum()))


def test_cap_moves_some_hashed_levels_of_every_part():
    from invr import params
    from invr.config import PART_NAMES
    cfg = _cfg(CAP)
    for name in PART_NAMES:
        spec = params.part_grid_spec(cfg, name)
        off, n = params.vertex_layout(spec, CAP)
        moved = [l for l in range(16) if off[l] >= 0]
        assert 0 < len(moved) < spec['L'] - spec['start_hash'] and n > 0, (name, moved)


def test_frame_with_vertex_tables_equals_frame_without(frame):
    from invr import params
    off = _net(0)
    on = _net(CAP)
    ref = _render(off, frame)
    assert float(ref['acc_map'].max()) > 0.5 and float(ref['raw'].abs().sum()) > 0         # (the frame shows the body)
    out = _render(on, frame)
    # the tables were built and handed over: every part's grid reads some levels through them
    m = on.model_struct([])
    for i, pn in enumerate(on.tpose_human.part_networks):
        e = pn.embedder
        assert m.part[i].grid.vertex_rows == CAP and m.part[i].grid.row_sums == e.vertex_sums(CAP).data_ptr(), i
        assert e.vertex_sums(CAP).numel() == e.row_sums().numel() + params.vertex_layout(e.spec, CAP)[1]
        assert e.derived_bytes() > 4 * e.row_sums().numel()
    m0 = off.model_struct([])
    assert all(m0.part[i].grid.vertex_rows == 0 for i in range(5))
    _same(out, ref, 'tables on / off')
    # the switch is read per render
    on.cfg['eval_vertex_rows'] = 0
    assert all(on.model_struct([]).part[i].grid.vertex_rows == 0 for i in range(5))
    _same(_render(on, frame), ref, 'switched off')


def test_vertex_tables_follow_an_in_place_table_change(frame):
    net = _net(CAP)
    before = _render(net, frame)
    e = net.tpose_human.part_networks[0].embedder
    vs_old = e.vertex_sums(CAP)
    with torch.no_grad():
        e.hash.data.mul_(-0.5)                                                  # (through .data: the version counter does not see it)
    e.invalidate_row_sums()
    after = _render(net, frame)
    assert e.vertex_sums(CAP) is not vs_old
    assert not torch.equal(after['raw'], before['raw']), 'the changed table does not show in the frame'
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    fresh = _net(CAP, sd)
    _same(after, _render(fresh, frame), 'changed in place / fresh network')
    _same(after, _render(_net(0, sd), frame), 'changed in place / fresh network without tables')
