"""Recorded facts of the reference's drop-in seam, from the IMPORTED reference (run where the reference checkout exists, with the
stand-ins of make_golden.py) -> tests/golden/reference_io.json, read by tests/test_reference_plugin.py:
  * cfg         — the reference's parsed config (configs/inb/inb_377.yaml, N_samples 16, 2^12-row tables) with
                  network_module / renderer_module set to the invr.plugin modules, as its factories see it
  * state_dict  — [name, shape, dtype] of every entry of the reference's OWN network class at that config, in order, and the values
                  of its small integer buffers (constructor arithmetic)
  * checkpoint  — what the reference's net_utils.save_model wrote (file names, top-level keys in order) and what its load_network /
                  load_model returned on those files
Only settings, names and recorded results are stored; no reference source."""
import json
import os
import sys
import tempfile

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import make_golden as MG      # noqa: E402

OUT = os.path.join(HERE, 'reference_io.json')
PLUGIN_OPTS = ['network_module', 'invr.plugin.network', 'renderer_module', 'invr.plugin.renderer']
SMALL_BUFFER = 4096           # integer buffers up to this many elements are stored with their values


def plain(x):
    if hasattr(x, 'items'):
        return {k: plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def main():
    rcfg = MG.import_reference(16, PLUGIN_OPTS)
    cfg = plain(rcfg)
    from lib.networks.make_network import make_network
    from lib.utils import net_utils
    rcfg.network_module = 'lib.networks.bw_deform.inb_part_network_multiassign'
    torch.manual_seed(0)
    ref_net = make_network(rcfg)
    sd = ref_net.state_dict()
    entries = [[k, list(v.shape), str(v.dtype)] for k, v in sd.items()]
    int_buffers = {k: v.flatten().tolist() for k, v in sd.items() if not v.dtype.is_floating_point and v.numel() <= SMALL_BUFFER}

    class Rec:
        def state_dict(self):
            return {'step': 3}

        def load_state_dict(self, s):
            self.s = s
    opt = torch.optim.Adam(ref_net.parameters())
    sch = torch.optim.lr_scheduler.ExponentialLR(opt, 0.9)
    ck = {}
    for name, epoch, last in (('last', 4, True), ('epoch', 7, False)):
        d = tempfile.mkdtemp()
        net_utils.save_model(ref_net, opt, sch, Rec(), d, epoch, last=last)
        files = sorted(os.listdir(d))
        assert len(files) == 1, files
        top = torch.load(os.path.join(d, files[0]), map_location='cpu')
        ck[name] = {'epoch': epoch, 'last': last, 'files': files, 'keys': list(top.keys()),
                    'load_network_returns': net_utils.load_network(ref_net, d),
                    'load_model_returns': net_utils.load_model(ref_net, opt, sch, Rec(), d)}
    rec = {'cfg': cfg, 'state_dict': entries, 'int_buffers': int_buffers, 'checkpoint': ck}
    with open(OUT, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=False)
        f.write('\n')
    print('wrote', OUT, os.path.getsize(OUT), 'bytes;', len(entries), 'state_dict entries,', len(int_buffers), 'integer buffers')


if __name__ == '__main__':
    main()
