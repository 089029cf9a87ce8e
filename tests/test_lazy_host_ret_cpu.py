"""CPU: dict semantics of the eval return object (invr.renderer.LazyHostRet): the reference's callers treat the return of
Renderer.render as a plain dict of host tensors (evaluators/if_nerf.py:77, visualizers/if_nerf.py:24 index it; run.py iterates it)."""
import copy
import pickle

import torch

from invr.renderer import LazyHostRet


def make():
    host = {'rgb_map': torch.arange(6.).reshape(1, 2, 3), 'acc_map': torch.ones(1, 2)}
    lazy = {'raw': torch.arange(8.).reshape(1, 2, 4), 'occ': torch.arange(8.).reshape(1, 2, 4)[..., 3:]}      # (occ: a strided view, as the renderer hands it over)
    return LazyHostRet(host, lazy, pin=False), host, lazy


def test_access_by_key_fetches_only_that_key():
    r, host, lazy = make()
    assert set(r.pending()) == {'raw', 'occ'} and len(r) == 4 and 'raw' in r and 'nope' not in r
    assert r['rgb_map'] is host['rgb_map'] and set(r.pending()) == {'raw', 'occ'}
    assert torch.equal(r['occ'], lazy['occ']) and r['occ'].is_contiguous() and r.pending() == ('raw',)
    assert r.get('nope', 5) == 5 and torch.equal(r.get('raw'), lazy['raw']) and r.pending() == ()


def test_whole_dict_views_fetch_everything():
    for use in (lambda r: dict(r), lambda r: {k: v for k, v in r.items()}, lambda r: {k: r[k] for k in r}, lambda r: r.copy(),
                lambda r: dict(zip(r.keys(), r.values())), lambda r: copy.deepcopy(r), lambda r: pickle.loads(pickle.dumps(r))):
        r, host, lazy = make()
        d = use(r)
        assert type(d) is dict and set(d) == {'rgb_map', 'acc_map', 'raw', 'occ'}
        assert torch.equal(d['raw'], lazy['raw']) and torch.equal(d['occ'], lazy['occ'])


def test_pop_eq_repr():
    r, host, lazy = make()
    assert 'on the device' in repr(r)
    assert torch.equal(r.pop('raw'), lazy['raw']) and 'raw' not in r and len(r) == 3
    assert r.pop('nope', None) is None
    r2, _, _ = make()
    r2.pop('raw')
    assert set(r.keys()) == set(r2.keys())


def test_renderer_bounds_the_memory_behind_unread_dicts():
    """Renderer._track_lazy: dicts whose raw / occ nobody read are completed on the host, oldest first, once the tensors they keep
    alive exceed lazy_device_budget (device_bytes counts CUDA storages; on the CPU the bookkeeping is exercised with a stand-in)."""
    from invr.renderer import Renderer

    class R(LazyHostRet):
        def device_bytes(self):
            return 0 if self._pending is not None else sum(v.numel() * 4 for k, v in self._lazy.items() if k == 'raw')
    r = Renderer.__new__(Renderer)
    r.lazy_device_budget, r._lazy_live = 2 * 8 * 4, []
    rets = []
    for i in range(5):
        host = {'rgb_map': torch.zeros(1, 2, 3)}
        raw = torch.full((1, 2, 4), float(i))
        rets.append(r._track_lazy(R(host, {'raw': raw, 'occ': raw[..., 3:]}, pin=False)))
    assert [x.pending() for x in rets[:3]] == [(), (), ()] and all(set(x.pending()) == {'raw', 'occ'} for x in rets[3:])
    assert all(float(x['raw'][0, 0, 0]) == i for i, x in enumerate(rets))            # values survive either way
    del rets
    r._track_lazy(R({}, {'raw': torch.zeros(1, 2, 4)}, pin=False))
    assert len(r._lazy_live) == 1                                                  # dead dicts are dropped from the book


def test_lazy_train_ret_dict_views_see_thunks_and_lazy_tensors():
    from invr.autograd import LazyTrainRet
    calls = []

    def mat():
        calls.append(1)
        return {'resd': torch.ones(1, 2, 3), 'tocc': torch.zeros(1, 2, 1)}
    mk = lambda: LazyTrainRet({'rgb_map': torch.zeros(1, 2, 3)}, ['resd', 'tocc'], mat, {'offset_loss': lambda: torch.tensor(2.0)})
    r = mk()
    assert len(r) == 4 and 'offset_loss' in r and 'resd' in r and not calls
    assert set(dict(r)) == {'rgb_map', 'resd', 'tocc', 'offset_loss'} and len(calls) == 1
    for use in (lambda x: {k: v for k, v in x.items()}, lambda x: dict(zip(x.keys(), x.values())), lambda x: {k: x[k] for k in x},
                lambda x: x.copy(), lambda x: copy.deepcopy(x), lambda x: pickle.loads(pickle.dumps(x))):
        d = use(mk())
        assert type(d) is dict and set(d) == {'rgb_map', 'resd', 'tocc', 'offset_loss'} and float(d['offset_loss']) == 2.0
    r = mk()
    assert float(r.pop('offset_loss')) == 2.0 and 'offset_loss' not in r and len(r) == 3


def test_lane_raw_buffer_is_reused_only_when_unreferenced():
    """Renderer lanes (in_flight > 1) hand the previous frame's raw buffer to the next frame only when no dict / tensor views it any
    more (storage use count) — a caller that kept `ret['raw']` keeps its data."""
    from invr.renderer import _Lane
    lane = _Lane.__new__(_Lane)
    lane.raw_buf = None
    dev = torch.device('cpu')
    a = lane.raw_buffer(1000, dev)
    assert a.numel() >= 1000 and lane.raw_buffer(900, dev) is a                     # nobody else references it: reused
    view = a[:400].view(100, 4)                                                    # (what a returned dict holds)
    b = lane.raw_buffer(900, dev)
    assert b is not a and b.untyped_storage().data_ptr() != a.untyped_storage().data_ptr()
    del view, a
    assert lane.raw_buffer(900, dev) is b
    c = lane.raw_buffer(10 * b.numel(), dev)                                       # a larger frame: a larger buffer
    assert c is not b and c.numel() >= 10 * b.numel()


class _StubPending:
    """a frame still in flight (what Renderer.in_flight > 1 hands to LazyHostRet): result() joins it"""
    def __init__(self):
        self.joined = 0

    def done(self):
        return self.joined > 0

    def result(self):
        self.joined += 1
        raw = torch.arange(8.).reshape(1, 2, 4)
        return {'rgb_map': torch.arange(6.).reshape(1, 2, 3), 'acc_map': torch.ones(1, 2)}, {'raw': raw, 'occ': raw[..., 3:]}


def test_first_whole_dict_access_of_a_frame_in_flight_has_every_key():
    """keys() / items() / values() / iteration / dict(ret) / == / copy / pickling on a dict whose frame is still in flight
    must join the frame BEFORE deciding what to fetch — the first such access used to return rgb_map / acc_map only."""
    full = {'rgb_map', 'acc_map', 'raw', 'occ'}
    uses = (lambda r: dict(r), lambda r: dict(r.items()), lambda r: {k: r[k] for k in r}, lambda r: r.copy(), lambda r: dict(zip(r.keys(), r.values())),
            lambda r: copy.deepcopy(r), lambda r: pickle.loads(pickle.dumps(r)), lambda r: dict(zip(list(r), r.values())))
    for use in uses:
        p = _StubPending()
        r = LazyHostRet({}, {}, pin=False, pending=p, keys=sorted(full))
        assert len(r) == 4 and r.in_flight() and set(r.pending()) == full and p.joined == 0
        d = use(r)
        assert p.joined == 1 and type(d) is dict and set(d) == full, (set(d), full)
        assert all(not v.is_cuda for v in d.values()) and r.pending() == ()
    p = _StubPending()
    r = LazyHostRet({}, {}, pin=False, pending=p, keys=sorted(full))
    r2, _, _ = make()
    assert set(r.keys()) == full and (r == r) and set(r2.keys()) == full
    r = LazyHostRet({}, {}, pin=False, pending=_StubPending(), keys=sorted(full))
    r.fetch()
    assert r.pending() == () and set(dict.keys(r)) == full


def test_lazy_dev_ret_joins_once_and_becomes_the_plain_dict():
    """LazyDevRet (eval_to_cpu = False with frames in flight): len() / `in` / in_flight() answer from the promise without joining; every
    whole-dict use joins the frame exactly once and sees every key."""
    from invr.renderer import LazyDevRet
    full = {'rgb_map', 'acc_map', 'raw', 'occ'}

    class P(_StubPending):
        def result(self):
            maps, lazy = _StubPending.result(self)
            return dict(maps, **lazy), {}
    uses = (lambda r: dict(r), lambda r: dict(r.items()), lambda r: {k: r[k] for k in r}, lambda r: r.copy(), lambda r: dict(zip(r.keys(), r.values())),
            lambda r: copy.deepcopy(r), lambda r: pickle.loads(pickle.dumps(r)), lambda r: dict(zip(list(r), r.values())))
    for use in uses:
        p = P()
        r = LazyDevRet(p, sorted(full))
        assert len(r) == 4 and 'raw' in r and 'nope' not in r and r.in_flight() and p.joined == 0
        d = use(r)
        assert p.joined == 1 and type(d) is dict and set(d) == full, (set(d), full)
        assert not r.in_flight() and len(r) == 4 and set(dict.keys(r)) == full
        dict(r), r['raw'], r.get('occ')
        assert p.joined == 1
    p = P()
    r = LazyDevRet(p, sorted(full))
    assert torch.equal(r['occ'], torch.arange(8.).reshape(1, 2, 4)[..., 3:]) and p.joined == 1


def _lazy_dicts():
    """one of each class (LazyHostRet joined and in flight) -> (dict, the keys it must show, the count of its resolving calls, a key it still owes)"""
    from invr.renderer import LazyDevRet
    from invr.autograd import LazyTrainRet
    full = ('acc_map', 'occ', 'raw', 'rgb_map')
    host = make()[0]
    ph = _StubPending()
    flying = LazyHostRet({}, {}, pin=False, pending=ph, keys=full)

    class P(_StubPending):
        def result(self):
            maps, lazy = _StubPending.result(self)
            return dict(maps, **lazy), {}
    pd = P()
    dev = LazyDevRet(pd, full)
    calls = []
    train = LazyTrainRet({'rgb_map': torch.zeros(1, 2, 3)}, ['resd', 'tocc'],
                         lambda: calls.append(1) or {'resd': torch.ones(1, 2, 3), 'tocc': torch.zeros(1, 2, 1)}, {'offset_loss': lambda: torch.tensor(2.0)})
    return ((host, set(full), lambda: 1, 'raw'), (flying, set(full), lambda: ph.joined, 'raw'), (dev, set(full), lambda: pd.joined, 'raw'),
            (train, {'rgb_map', 'resd', 'tocc', 'offset_loss'}, lambda: len(calls), 'tocc'))


def test_setdefault_popitem_reversed_ne_or_see_the_resolved_dict():
    """the views the three classes did not cover before lazyret.LazyDict: each of them resolves what is promised first"""
    n = len(_lazy_dicts())
    for i in range(n):
        r, full, resolved, k = _lazy_dicts()[i]
        assert not dict.__contains__(r, k) and k in r
        v = r.setdefault(k, 'default')
        assert torch.is_tensor(v) and dict.__getitem__(r, k) is v and r.setdefault('extra', 7) == 7 and len(r) == len(full) + 1

        r, full, resolved, _ = _lazy_dicts()[i]
        k, v = r.popitem()
        assert resolved() == 1 and k in full and torch.is_tensor(v) and set(dict.keys(r)) == full - {k} and len(r) == len(full) - 1

        r, full, resolved, _ = _lazy_dicts()[i]
        assert set(reversed(r)) == full and resolved() == 1 and list(reversed(r)) == list(r)[::-1]

        r, full, resolved, _ = _lazy_dicts()[i]
        same = dict(_lazy_dicts()[i][0])
        assert set(same) == full
        assert (r != {}) is True and resolved() == 1 and set(dict.keys(r)) == full
        assert (r != r) is False and (r == r) is True
        assert (r != {k: dict.__getitem__(r, k) for k in full}) is False             # (the same tensor objects: dict compares by identity first)

        r, full, resolved, _ = _lazy_dicts()[i]
        d = r | {'extra': 1}
        assert type(d) is dict and set(d) == full | {'extra'} and resolved() == 1
        r, full, resolved, _ = _lazy_dicts()[i]
        d = {'extra': 1} | r
        assert type(d) is dict and set(d) == full | {'extra'} and list(d)[0] == 'extra' and resolved() == 1
        r, full, resolved, _ = _lazy_dicts()[i]
        r |= {'extra': 1}
        assert set(dict.keys(r)) == full | {'extra'} and len(r) == len(full) + 1 and resolved() == 1


def test_lazy_train_ret_thunk_and_present_keys_do_not_materialise():
    """The trainer's objective reads rgb_map and the fused regulariser scalars every iteration: neither may trigger the read-back of
    resd / tpts / tocc / oresd, which synchronises with the device."""
    from invr.autograd import LazyTrainRet
    calls = []

    def mat():
        calls.append(1)
        return {'resd': torch.ones(1, 2, 3), 'tocc': torch.zeros(1, 2, 1)}
    r = LazyTrainRet({'rgb_map': torch.zeros(1, 2, 3)}, ['resd', 'tocc'], mat, {'offset_loss': lambda: torch.tensor(2.0)})
    assert r['rgb_map'].shape == (1, 2, 3) and float(r['offset_loss']) == 2.0 and float(r.get('offset_loss')) == 2.0
    assert 'resd' in r and 'pair_loss' not in r and r.get('pair_loss') is None and len(r) == 4
    assert not calls
    assert r['tocc'].shape == (1, 2, 1) and r['resd'].shape == (1, 2, 3) and len(calls) == 1 and len(r) == 4


def test_survivor_capacity_policy():
    """The survivor capacity of an eval frame's workspace, stated once in invr.renderer: the bound of a frame under the hint, the
    overflow flag stats[6] and its error, the grow-only update with each path's head-room."""
    import pytest
    from invr import renderer as R
    n_samp = 512 * 512 * 128
    assert R.cap_bound(n_samp, None) == n_samp // 4                      # no hint: a quarter of the ray-samples
    assert R.cap_bound(64 * 64 * 32, None) == 65536                      # ... but no less than 65536
    assert R.cap_bound(1000, None) == 1000                               # ... and no more than the frame has
    assert R.cap_bound(n_samp, 10) == 65536                              # a small hint
    assert R.cap_bound(n_samp, 3000000) == 3000000
    assert R.cap_bound(n_samp, n_samp + 1) == n_samp                     # a hint above n_samp
    assert (R.CAP_HEADROOM_SYNC, R.CAP_HEADROOM_LANE, R.CAP_HEADROOM_FIRST) == (1.5, 1.25, 1.2)
    stats = torch.zeros(16, dtype=torch.int32)
    stats[0] = 1000000
    assert R.cap_grown(None, stats, R.CAP_HEADROOM_SYNC) == 1500000 + 65536
    assert R.cap_grown(None, stats, R.CAP_HEADROOM_LANE) == 1250000 + 65536
    assert R.cap_grown(10, stats, R.CAP_HEADROOM_LANE) == 1250000 + 65536
    assert R.cap_grown(5000000, stats, R.CAP_HEADROOM_SYNC) == 5000000   # grow-only
    assert R.cap_grown(5000000, stats, R.CAP_HEADROOM_LANE) == 5000000
    assert int(R.CAP_HEADROOM_FIRST * R.cap_grown(None, stats, R.CAP_HEADROOM_LANE)) == int(1.2 * (1250000 + 65536))
    assert not R.cap_overflowed(stats)
    R.cap_check(stats)
    stats[6] = 37
    assert R.cap_overflowed(stats)
    with pytest.raises(RuntimeError, match=r'stats\[6\] = 37.*workspace overflow'):
        R.cap_check(stats)
