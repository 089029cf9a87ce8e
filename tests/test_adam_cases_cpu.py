"""CPU, no kernel involved: the checker of the fused Adam step (tests/adam_cases.py) held to account on its own.  torch's own fp32 CPU
Adam must meet the accepted rule on every input kind and size class — what validates the rule independently of the code under test —
and the rule must see a constant that is off by parts in 10^5."""
import numpy as np
import pytest
import torch

from tests import adam_cases as AC

RULE_N = [1, 3, 5, 1025, 4099, 16385, 65536]


@pytest.mark.parametrize('kind', AC.KINDS)
def test_torch_fp32_adam_meets_the_accepted_rule(kind):
    """torch.optim.Adam in fp32 on the CPU (foreach=False, state injected) — another order of the same operations, separate multiplies
    where the kernel fuses — stays within 2 E of the float64 reference for every input kind, size class, step count and weight decay.
    Prints its K (profiles/adam_step_headroom.md)."""
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for i, n in enumerate(RULE_N):
        for j, step in enumerate(AC.STEPS):
            if kind == 'first' and step != 1:
                continue
            for wd in AC.WDS:
                sc = AC.scalars(AC.LRS[(i + j) % 3], wd, step)
                p, g, m, v = AC.make_inputs(kind, n, sc, seed=3)
                ref = AC.reference(p, g, m, v, sc)
                out = AC.torch_adam32(p, g, m, v, sc)
                ks = AC.headroom(out, ref)
                for k in 'pmv':
                    assert ks[k] <= AC.ACCEPT, (kind, n, step, wd, k, ks[k])
                    worst[k] = max(worst[k], ks[k])
                assert (out['v'] >= 0).all()
    print('ADAM-K rule %s torch32 p=%.3f m=%.3f v=%.3f' % (kind, worst['p'], worst['m'], worst['v']))


def test_inputs_are_the_regimes_they_are_named_after():
    sc = AC.scalars(5e-4, 0.0, 1000)
    for kind in AC.KINDS:
        p, g, m, v = AC.make_inputs(kind, 4099, sc)
        assert all(x.dtype == torch.float32 and x.shape == (4099,) and torch.isfinite(x).all() for x in (p, g, m, v)) and (v >= 0).all()
        assert torch.equal(p, AC.make_inputs(kind, 4099, sc)[0])                # deterministic
    p, g, m, v = AC.make_inputs('first', 4099, sc)
    assert not m.any() and not v.any() and g.abs().min() > 0
    p, g, m, v = AC.make_inputs('zeros', 4099, sc)
    assert not g.any() and (m == 0).sum() >= 2000 and (m != 0).sum() >= 2000 and ((v > 0) & (v < 1.17e-38)).sum() >= 1000
    p, g, m, v = AC.make_inputs('tiny', 4099, sc)
    assert (v > 0).all() and v.max() < 1.17e-38 and g.abs().max() < 1e-19            # subnormal second moments; sqrt(v) far below eps
    p, g, m, v = AC.make_inputs('spike', 4099, sc)
    assert ((g.abs() / v.sqrt()) >= 99).all() and ((g.abs() / v.sqrt()) <= 1.01e4).all()
    p, g, m, v = AC.make_inputs('wide', 4099, sc)
    assert p.abs().max() / p.abs().min() > 2.0 ** 70 and v.max() / v.min() > 2.0 ** 70
    p, g, m, v = AC.make_inputs('cancel', 4099, sc)
    r = AC.reference(p, g, m, v, sc)
    assert ((g - m).abs() <= 1e-5 * m.abs()).all() and (r['p'].abs() <= 0.02 * p.double().abs()).all()
    assert AC.make_inputs('training', 64, sc, n_grad=4)[1].shape == (4,)


def test_rule_sees_a_constant_that_is_off_by_parts_in_1e5():
    """w2 = 1.0f - 0.999f (1.3e-5 off 0.001, the mistake tests/test_gpu_parity.py records) evaluated in float64 exceeds the rule on
    fresh moments by far; the exact result rounded to fp32 sits inside E."""
    sc = AC.scalars(5e-4, 0.0, 1)
    p, g, m, v = AC.make_inputs('first', 4099, sc)
    ref = AC.reference(p, g, m, v, sc)
    bad = AC.reference(p, g, m, v, dict(sc, w2=float(np.float32(1.0) - np.float32(0.999))))
    ks = AC.headroom(bad, ref)
    assert ks['v'] > 50 and ks['p'] > 5, ks
    assert max(AC.headroom({k: ref[k].float() for k in 'pmv'}, ref).values()) <= 1.0


def test_canaries_show_a_write_and_a_shift():
    c = AC.Carved(torch.arange(5.0), 'cpu', mis=1)
    assert c.t.data_ptr() % 16 == 4 and c.unchanged() and torch.equal(c.cpu(), torch.arange(5.0))
    c.buf[c.o + c.n] = 0.0
    assert not c.canaries_intact()
    c = AC.Carved(torch.arange(5.0), 'cpu')
    c.buf[c.o - 1] = float('nan')
    assert c.t.data_ptr() % 16 == 0 and not c.canaries_intact()
    c = AC.Carved(torch.arange(5.0), 'cpu')
    c.t[4] = 5.0
    assert c.canaries_intact() and not c.unchanged()
