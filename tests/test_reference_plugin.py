"""Drop-in seam against what the reference's own factories and checkpoint I/O do, as recorded from the imported reference
(tests/golden/make_golden_plugin.py -> tests/golden/reference_io.json: its parsed config, its network's state_dict layout, the
files and keys its save_model wrote and what its load_network / load_model returned on them).

The factories are one line each (lib/networks/make_network.py:5-8, lib/networks/renderer/make_renderer.py:5-16): import the yaml's
module string, call Network() / Renderer(network); the host's parsed config is the module lib.config's `cfg`.  The seam runs in a
subprocess because adopting the host config is process-wide."""
import json
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
RECORD = os.path.join(ROOT, 'tests', 'golden', 'reference_io.json')
TABLE_LOG2 = 12                           # make_golden.TABLE_LOG2: the table size of the recorded config

SCRIPT = r'''
import importlib, json, sys, types
sys.path.insert(0, %(root)r)
rec = json.load(open(%(record)r))
cfg = rec['cfg']
# the host application: its parsed config is lib.config.cfg (a nested mapping) before the factories import anything
host = types.ModuleType('lib.config'); host.cfg = cfg
lib = types.ModuleType('lib'); lib.config = host
sys.modules['lib'], sys.modules['lib.config'] = lib, host
import torch
net = importlib.import_module(cfg['network_module']).Network()          # make_network(cfg)
import invr
from invr.network import Network
from invr.renderer import Renderer
assert type(net) is Network, type(net)
assert invr.config.cfg.N_samples == 16 and invr.config.cfg.smpl_thresh == cfg['smpl_thresh']
split = cfg.get('test', {})
module = split['renderer_module'] if 'renderer_module' in split else cfg['renderer_module']
r = importlib.import_module(module).Renderer(net)                       # make_renderer(cfg, net)
assert type(r) is Renderer and r.net is net
# checkpoint interchange with the reference's own network class: the same entries, in the same order, with the same shapes / dtypes
sd = net.state_dict()
assert [e[0] for e in rec['state_dict']] == list(sd.keys())
ref_sd = {}
for k, shape, dtype in rec['state_dict']:
    assert list(sd[k].shape) == shape and str(sd[k].dtype) == dtype, (k, tuple(sd[k].shape), shape, sd[k].dtype, dtype)
    ref_sd[k] = torch.rand(shape).to(getattr(torch, dtype.split('.')[-1])) if k not in rec['int_buffers'] else \
        torch.tensor(rec['int_buffers'][k], dtype=getattr(torch, dtype.split('.')[-1])).view(shape)
for k, v in rec['int_buffers'].items():                                  # constructor arithmetic of the integer buffers
    assert sd[k].flatten().tolist() == v, k
net.load_state_dict(ref_sd, strict=True)
for k, v in ref_sd.items():
    assert torch.equal(net.state_dict()[k], v), k
print('PLUGIN_OK', len(sd))
'''


def test_reference_factories_pick_up_invr_plugin():
    env = dict(os.environ, PYTHONBREAKPOINT='0')
    r = subprocess.run([sys.executable, '-c', SCRIPT % {'root': ROOT, 'record': RECORD}], capture_output=True, text=True, env=env,
                       timeout=600)
    assert 'PLUGIN_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


class _Rec:
    def state_dict(self):
        return {'step': 3}

    def load_state_dict(self, s):
        self.s = s


def _reference_layout_state_dict(rec, seed):
    """a state dict laid out as the reference's network writes it (recorded names, order, shapes, dtypes), random values"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, shape, dtype in rec['state_dict']:
        dt = getattr(torch, dtype.split('.')[-1])
        if k in rec['int_buffers']:
            out[k] = torch.tensor(rec['int_buffers'][k], dtype=dt).view(shape)
        elif dt.is_floating_point:
            out[k] = torch.rand(shape, generator=g).to(dt)
        else:
            out[k] = torch.randint(0, 1000, shape, generator=g).to(dt)
    return out


def test_checkpoints_interchange_with_reference_io():
    import invr  # noqa: F401
    from invr import driver
    from invr.network import Network
    from invr.config import make_cfg
    rec = json.load(open(RECORD))
    ck = rec['checkpoint']
    mine = Network(cfg=make_cfg(table_log2=TABLE_LOG2, N_samples=16))
    opt = torch.optim.Adam(mine.parameters())
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9)
    # reference -> ours: a checkpoint as the reference's save_model writes it (file name, top-level keys in order) loads into the
    # drop-in network, and the epoch that comes back is the one the reference's own load_network returned on such a file
    d = tempfile.mkdtemp()
    ref_sd = _reference_layout_state_dict(rec, 0)
    top = {'net': ref_sd, 'optim': opt.state_dict(), 'scheduler': sch.state_dict(), 'recorder': _Rec().state_dict(), 'epoch': ck['last']['epoch']}
    assert sorted(top) == sorted(ck['last']['keys'])
    torch.save({k: top[k] for k in ck['last']['keys']}, os.path.join(d, ck['last']['files'][0]))
    assert driver.load_network(mine, d) == ck['last']['load_network_returns']
    for (k, a), (k2, b) in zip(ref_sd.items(), mine.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    # ours -> reference: driver.save_model writes the file name and top-level layout the reference's save_model writes, so its
    # load_network / load_model read it as they read their own (recorded: they returned epoch + 1)
    d2 = tempfile.mkdtemp()
    with torch.no_grad():
        for p in mine.parameters():
            if p.dtype.is_floating_point:
                p.add_(0.25)
    e = ck['epoch']
    driver.save_model(mine, opt, sch, _Rec(), d2, e['epoch'], last=e['last'])
    assert sorted(os.listdir(d2)) == e['files']
    got = torch.load(os.path.join(d2, e['files'][0]), map_location='cpu')
    assert list(got.keys()) == e['keys']
    assert got['epoch'] + 1 == e['load_network_returns'] == e['load_model_returns']
    assert [[k, list(v.shape), str(v.dtype)] for k, v in got['net'].items()] == rec['state_dict']
    for (k, a), (k2, b) in zip(got['net'].items(), mine.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    opt.load_state_dict(got['optim'])
    sch.load_state_dict(got['scheduler'])
    assert got['recorder'] == {'step': 3}
    # and the drop-in's own loader reads it back, as it reads the reference's files
    back = Network(cfg=make_cfg(table_log2=TABLE_LOG2, N_samples=16))
    assert driver.load_network(back, d2) == e['load_network_returns']
    for (k, a), (k2, b) in zip(back.state_dict().items(), mine.state_dict().items()):
        assert torch.equal(a, b), k
