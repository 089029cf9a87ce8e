"""GPU: the four ways Renderer.render hands an eval frame back — on the caller's stream or on a lane with frames in flight, outputs
moved to the host (LazyHostRet) or left on the device (plain dict / LazyDevRet) — return the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from invr.network import Network            # noqa: E402
from invr.renderer import Renderer, LazyHostRet, LazyDevRet          # noqa: E402

DEV = 'cuda:0'
KEYS = ('rgb_map', 'acc_map', 'raw', 'occ')


def test_eval_return_paths_agree_bit_for_bit(small_setup):
    cfg, sd, batch, extras = small_setup
    net = Network(cfg=cfg)
    net.load_state_dict(sd, strict=True)
    net = net.to(DEV).eval()
    gb = {k: v.to(DEV) for k, v in batch.items()}

    def maps_first(ret):
        """a host variant: reading the maps leaves raw / occ on the device"""
        assert type(ret) is LazyHostRet
        got = {k: ret[k] for k in ('rgb_map', 'acc_map')}
        assert set(ret.pending()) == {'raw', 'occ'} and ret.device_bytes() > 0
        got.update({k: ret[k] for k in ('raw', 'occ')})
        assert ret.pending() == () and all(not v.is_cuda for v in got.values())
        return got

    with torch.no_grad():
        r = Renderer(net)
        ref = maps_first(r.render(dict(gb)))
        assert float(ref['rgb_map'].abs().max()) > 0 and float(ref['raw'].abs().max()) > 0

        r = Renderer(net)
        r.eval_to_cpu = False
        dev = r.render(dict(gb))
        assert type(dev) is dict and int(r.last_stats[6]) == 0
        for k in KEYS:
            assert dev[k].is_cuda and torch.equal(dev[k].cpu(), ref[k]), k

        for to_cpu in (True, False):
            r = Renderer(net)
            r.in_flight, r.eval_to_cpu = 3, to_cpu
            rets = [r.render(dict(gb)) for _ in range(4)]              # the fourth lands on the first one's lane
            assert all(type(x) is (LazyHostRet if to_cpu else LazyDevRet) for x in rets)
            assert rets[3]._pending is not None and len(rets[3]) == 4 and 'occ' in rets[3]          # not joined yet
            for i in (3, 1, 2, 0):
                got = maps_first(rets[i]) if to_cpu else rets[i]
                for k in KEYS:
                    assert got[k].is_cuda != to_cpu and torch.equal(got[k].cpu(), ref[k]), (to_cpu, i, k)
                assert not rets[i].in_flight() and type(dict(rets[i])) is dict
            r.flush(release=True)
