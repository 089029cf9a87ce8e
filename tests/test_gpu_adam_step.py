"""GPU: the fused Adam step (csrc/k_optim.hip: k_adam, k_adam_advance) called through the C-ABI exactly as FusedAdam.step does — an
InvrAdamTensor table as device bytes and the two int32 chunk tables — against the float64 reference of tests/adam_cases.py, element
by element, every element of p, exp_avg and exp_avg_sq:

    |kernel - exact|  <=  2 E          E = one rounding (2^-24 relative, 2^-149 absolute) per fp32 operation of the update,
                                       propagated to first order in float64 from the reference's own intermediates

Nothing is fitted to the kernel.  Every array is carved from a larger buffer between 64 canary floats; canaries and the whole
gradient array must be bit-unchanged after every launch.  Each case prints K = max_e |x - exact| / E_x for the kernel and for
torch's own fp32 CPU Adam (profiles/adam_step_headroom.md keeps them).

Why element by element: the trajectory tests hold a tensor to 2e-6 of its maximum against another fp32 implementation.  One wrong
element at a tail, a row-scalar gradient read one row off, a constant that is 1.3e-5 off move a few elements by parts in 10^5 of
THOSE elements and nothing relative to the tensor's maximum.

tests/test_hostsim_adam_cpu.py runs the same bodies on the CPU wave machine (DEV switched to 'cpu')."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import adam_cases as AC          # noqa: E402  (checker only)
from invr import _abi                       # noqa: E402

DEV = 'cuda:0'
BETAS = (0.9, 0.999)
EPS = 1e-15


def sync():
    if DEV != 'cpu':
        torch.cuda.synchronize()


class Ten:
    """One tensor of a launch: canary-fenced p, g, m, v on the device and the scalars of its table entry."""

    def __init__(self, p, g, m, v, lr=5e-4, wd=0.0, step=1, shift=0, mis='', active=None, betas=BETAS):
        self.p, self.m, self.v = (AC.Carved(x, DEV, int(k in mis)) for k, x in (('p', p), ('m', m), ('v', v)))
        self.g = AC.Carved(g, DEV, int('g' in mis))
        self.n, self.shift, self.active = p.numel(), shift, active
        assert self.g.n << shift == self.n
        self.host = (p, g, m, v)
        self.set_step(lr, wd, step, betas)

    def set_step(self, lr, wd, step, betas=BETAS, bc=None):
        self.step = step
        self.sc = AC.scalars(lr, wd, step, betas, EPS, bc)

    def entry(self, e):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = self.p.ptr, self.g.ptr, self.m.ptr, self.v.ptr
        e.numel, e.lr, e.weight_decay, e.bc1, e.bc2_sqrt = self.n, self.sc['lr'], self.sc['wd'], self.sc['bc1'], self.sc['bc2s']
        e.active = None if self.active is None else self.active.data_ptr()
        e.grad_shift, e.step = self.shift, self.step

    def out(self):
        return {'p': self.p.cpu(), 'm': self.m.cpu(), 'v': self.v.cpu()}

    def grad_expanded(self, g=None):
        g = self.host[1] if g is None else g
        return g.repeat_interleave(1 << self.shift) if self.shift else g

    def reference(self, state=None, g=None):
        p, _, m, v = self.host if state is None else (state['p'], None, state['m'], state['v'])
        return AC.reference(p, self.grad_expanded(g), m, v, self.sc)

    def fences_hold(self, tag):
        for k in 'pmvg':
            assert getattr(self, k).canaries_intact(), (tag, k, 'canary overwritten')
        assert self.g.unchanged(), (tag, 'the gradient was written')

    def untouched(self):
        return self.p.unchanged() and self.m.unchanged() and self.v.unchanged()


def upload_table(tens):
    tab = (_abi.InvrAdamTensor * len(tens))()
    for e, t in zip(tab, tens):
        t.entry(e)
    return torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone().to(DEV)


def read_table(table, n):
    return (_abi.InvrAdamTensor * n).from_buffer_copy(bytes(table.cpu().numpy()))


def chunk_lists(tens):
    E = _abi.lib().invr_adam_chunk_elems()
    assert E == AC.CHUNK
    ct = [t for t, x in enumerate(tens) for _ in range((x.n + E - 1) // E)]
    ci = [c for x in tens for c in range((x.n + E - 1) // E)]
    return ct, ci


def adam_step(table, ct, ci, betas=BETAS, eps=EPS):
    ctd, cid = torch.tensor(ct, dtype=torch.int32).to(DEV), torch.tensor(ci, dtype=torch.int32).to(DEV)
    st = _abi.lib().invr_adam_step(C.c_void_p(table.data_ptr()), _abi.ptr(ctd, torch.int32), _abi.ptr(cid, torch.int32), len(ct),
                                   betas[0], betas[1], eps, _abi.stream_ptr())
    _abi.check(st)
    sync()


def adam_advance(table, n, betas=BETAS):
    _abi.check(_abi.lib().invr_adam_advance(C.c_void_p(table.data_ptr()), n, betas[0], betas[1], _abi.stream_ptr()))
    sync()


def launch(tens, order=None, split=None):
    """One invr_adam_step over `tens` (chunks in `order`; `split`: two launches, the chunk list cut there)."""
    table = upload_table(tens)
    ct, ci = chunk_lists(tens)
    if order is not None:
        ct, ci = [ct[i] for i in order], [ci[i] for i in order]
    parts = [(ct, ci)] if split is None else [(ct[:split], ci[:split]), (ct[split:], ci[split:])]
    for a, b in parts:
        adam_step(table, a, b)
    return table


def run_single(kind, n, step, wd, lr, shift=0, mis='', expand=False, seed=0):
    """One tensor, one launch -> (Ten, outputs).  expand: the row-scalar gradient handed over dense (grad_shift = 0)."""
    sc = AC.scalars(lr, wd, step, BETAS, EPS)
    p, g, m, v = AC.make_inputs(kind, n, sc, seed, n_grad=n >> shift)
    if expand:
        g, shift = g.repeat_interleave(1 << shift), 0
    t = Ten(p, g, m, v, lr, wd, step, shift, mis)
    launch([t])
    t.fences_hold((kind, n, shift, mis))
    return t, t.out()


# ---- 1. sizes x kinds ---------------------------------------------------------------------------------------------------------------
def _single(case):
    kind, n, step, wd, lr = case
    t, out = run_single(kind, n, step, wd, lr)
    AC.accept(AC.single_id(case), out, t.reference(), t.host, t.sc, family='single-' + kind)
    if kind == 'zeros' and wd == 0.0:
        p, _, m, v = t.host
        still = m == 0
        assert still.any() and (~still).any()
        # 0 / (sqrt(v') / bc2_sqrt + eps) is exactly 0: a row that never received a gradient does not move, bit for bit
        assert AC.same_bits(out['p'][still], p[still]) and (out['m'][still] == 0).all() and (out['v'][v == 0] == 0).all()
    if kind == 'tiny' and wd == 0.0:                                # (with weight decay g' = wd p dwarfs the tiny gradient)
        assert (out['v'] > 0).all() and float(out['v'].max()) < 1.2e-38, 'subnormal second moments flushed or blown up'
        assert not AC.same_bits(out['p'], t.host[0]), 'the eps-dominated update did not move p'


@pytest.mark.parametrize('case', AC.SINGLE_SMALL, ids=[AC.single_id(c) for c in AC.SINGLE_SMALL])
def test_adam_step_single(case):
    """Loop structure (unrolled 4 x 1024 strides, the single-float4 loop, the < 4 element tail, the 16384-element chunk edge), the
    production shapes, every input kind, steps 1 .. 10^5, weight decay, two learning rates."""
    _single(case)


@pytest.mark.parametrize('case', AC.SINGLE_LARGE, ids=[AC.single_id(c) for c in AC.SINGLE_LARGE])
def test_adam_step_single_large(case):
    _single(case)


def test_case_table_is_what_the_issue_lists():
    ns = {c[1] for c in AC.SINGLE}
    assert ns >= {1, 2, 3, 4, 5, 1023, 1024, 1025, 4095, 4096, 4097, 4099, 16383, 16384, 16385, 32771, 327920, 1216, 1088, 4480, 192, 96}
    for n in ns:
        assert ('training', n) in {(c[0], c[1]) for c in AC.SINGLE}
    for n in AC.ALL_KINDS_AT:
        assert {c[0] for c in AC.SINGLE if c[1] == n} == set(AC.KINDS)
    assert {c[2] for c in AC.SINGLE} == set(AC.STEPS) and {c[3] for c in AC.SINGLE} == {0.0, 0.01} and len({c[4] for c in AC.SINGLE}) == 2
    assert all(c[2] == 1 for c in AC.SINGLE if c[0] == 'first')
    assert {(c[0], c[1]) for c in AC.ROWS} == {(r, s) for r in AC.ROW_ROWS for s in (1, 2, 4)}


# ---- 2. row-scalar gradients --------------------------------------------------------------------------------------------------------
def _rows(case):
    rows, shift, kind, step, wd = case
    n = rows << shift
    t, out = run_single(kind, n, step, wd, 5e-4, shift=shift)
    assert t.g.n == rows                                           # exactly numel >> shift floats between the gradient's canaries
    AC.accept(AC.row_id(case), out, t.reference(), (t.host[0], t.grad_expanded(), t.host[2], t.host[3]), t.sc, family='rowscalar')
    _, dense = run_single(kind, n, step, wd, 5e-4, shift=shift, expand=True)
    for k in 'pmv':
        assert AC.same_bits(out[k], dense[k]), (AC.row_id(case), k, 'row-scalar and expanded gradient disagree')


@pytest.mark.parametrize('case', AC.ROWS_SMALL, ids=[AC.row_id(c) for c in AC.ROWS_SMALL])
def test_adam_step_row_scalar_gradient(case):
    """grad_shift > 0 (element i takes g[i >> shift]; shift 1: the scalar loop, shift >= 2: one gradient load per float4): the rule, and
    bit-identical to the same step on the expanded gradient.  A read behind the numel >> shift gradients lands in a canary."""
    _rows(case)


@pytest.mark.parametrize('case', AC.ROWS_LARGE, ids=[AC.row_id(c) for c in AC.ROWS_LARGE])
def test_adam_step_row_scalar_gradient_large(case):
    _rows(case)


# ---- 3. alignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', AC.ALIGN_N)
def test_adam_step_unaligned_arrays(n):
    """param / exp_avg / exp_avg_sq / grad each in turn, and all together, one float behind a 16-byte boundary (what a contiguous view
    t[1:] has): the scalar path, bit-identical to the float4 path of the aligned run."""
    case = ('training', n, 7, 0.01, 5e-4)
    t, want = run_single(*case)
    AC.accept('aligned-%d' % n, want, t.reference(), family='align')
    for which in AC.ALIGN_WHICH:
        _, out = run_single(*case, mis=which)
        for k in 'pmv':
            assert AC.same_bits(out[k], want[k]), (n, which, k)


@pytest.mark.parametrize('rows', [1, 3, 1025])
def test_adam_step_unaligned_parameters_with_row_scalar_gradient(rows):
    case = ('training', rows << 4, 2, 0.0, 5e-4)
    t, want = run_single(*case, shift=4)
    AC.accept('aligned-rows%d' % rows, want, t.reference(), family='align')
    for which in ('p', 'pmv', 'g', 'pmvg'):
        _, out = run_single(*case, shift=4, mis=which)
        for k in 'pmv':
            assert AC.same_bits(out[k], want[k]), (rows, which, k)


# ---- 4. one launch over many tensors --------------------------------------------------------------------------------------------------
# (kind, n, step, wd, lr, shift, misaligned arrays): the table FusedAdam builds — mixed sizes, shifts, alignments and scalars
MANY = [('training', 64 * 19, 7, 0.0, 5e-4, 0, ''), ('first', 17 * 64, 1, 0.0, 5e-4, 0, ''), ('training', 4099 * 16, 1000, 0.0, 5e-4, 4, ''),
        ('zeros', 1025 * 16, 2, 0.0, 1e-3, 4, ''), ('spike', 64 * 70, 2, 0.01, 5e-4, 0, ''), ('training', 3, 100000, 0.0, 1e-2, 0, ''),
        ('wide', 16385, 7, 0.0, 5e-4, 0, 'p'), ('tiny', 2 * 16384 + 3, 1000, 0.0, 2.5e-4, 0, ''), ('cancel', 4097, 2, 0.0, 5e-4, 0, 'g'),
        ('training', 1024 * 2, 7, 0.01, 5e-4, 1, ''), ('training', 1, 1, 0.0, 5e-4, 0, ''), ('first', 3 * 4, 1, 0.01, 5e-4, 2, 'pmv'),
        ('training', 32 * 32, 99999 + 1, 0.0, 5e-4, 0, 'pmvg'), ('wide', 1025 * 4, 1000, 0.01, 1e-3, 2, '')]


def many_tensors(active=None):
    tens = []
    for i, (kind, n, step, wd, lr, shift, mis) in enumerate(MANY):
        sc = AC.scalars(lr, wd, step, BETAS, EPS)
        p, g, m, v = AC.make_inputs(kind, n, sc, seed=i + 1, n_grad=n >> shift)
        tens.append(Ten(p, g, m, v, lr, wd, step, shift, mis, active=None if active is None else active[i]))
    return tens


def test_adam_step_many_tensors_any_chunk_order_one_or_two_launches():
    """The rule per tensor for one launch over 14 tensors; then the same bits with the chunk tables permuted and with the chunk list
    split over two launches (tools/exp_adam_overlap.py)."""
    tens = many_tensors()
    launch(tens)
    want = []
    for i, t in enumerate(tens):
        t.fences_hold(i)
        want.append(t.out())
        AC.accept('many-%d-%s-%d' % (i, MANY[i][0], t.n), want[-1], t.reference(), family='many')
    n_chunks = len(chunk_lists(tens)[0])
    assert n_chunks > len(tens) + 5
    perm = torch.randperm(n_chunks, generator=torch.Generator().manual_seed(5)).tolist()
    for tag, kw in (('permuted', dict(order=perm)), ('reversed', dict(order=list(range(n_chunks))[::-1])), ('split', dict(split=n_chunks // 3)),
                    ('permuted+split', dict(order=perm, split=n_chunks - 1))):
        again = many_tensors()
        launch(again, **kw)
        for i, t in enumerate(again):
            t.fences_hold((tag, i))
            out = t.out()
            for k in 'pmv':
                assert AC.same_bits(out[k], want[i][k]), (tag, i, k)


# ---- 5. active ----------------------------------------------------------------------------------------------------------------------------
def test_adam_step_active_flag_is_read_per_launch():
    """InvrAdamTensor.active: NULL or a device float; 0.0 -> the tensor is skipped (p, m, v bit for bit), anything else -> stepped.  The
    flag is read by every launch: flip it and step again."""
    flags = torch.tensor([0.0, 1.0], dtype=torch.float32).to(DEV)
    off, on = flags[0:1], flags[1:2]
    active = [(off, on, None)[i % 3] for i in range(len(MANY))]
    tens = many_tensors(active)
    table = launch(tens)
    state = []
    for i, t in enumerate(tens):
        t.fences_hold(i)
        if active[i] is off:
            assert t.untouched(), (i, 'a tensor whose active flag reads 0 was written')
            state.append({'p': t.host[0], 'm': t.host[2], 'v': t.host[3]})
        else:
            state.append(t.out())
            AC.accept('active-%d' % i, state[-1], t.reference(), family='active')
    assert sum(a is off for a in active) >= 4 and sum(a is on for a in active) >= 4
    flags.copy_(torch.tensor([1.0, 0.0]))                          # the same table, the same pointers: only the two device floats change
    sync()
    ct, ci = chunk_lists(tens)
    adam_step(table, ct, ci)
    for i, t in enumerate(tens):
        t.fences_hold(i)
        out = t.out()
        if active[i] is on:                                         # now reads 0
            for k in 'pmv':
                assert AC.same_bits(out[k], state[i][k]), (i, k, 'flag flipped to 0 but the tensor moved')
        else:
            AC.accept('active-flipped-%d' % i, out, t.reference(state[i]), family='active')


# ---- 6. invr_adam_advance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('betas', AC.ADVANCE_BETAS, ids=lambda b: 'b%g-%g' % b)
@pytest.mark.parametrize('n', AC.ADVANCE_N)
def test_adam_advance(n, betas):
    """Device-side step count and bias corrections: step + 1 exactly; bc1, bc2_sqrt within one fp32 ulp of the host's doubles (the
    device's double pow may differ from the host's in its last bit); no other byte of the table changes; entries whose active flag
    reads 0 do not change at all."""
    flags = torch.tensor([0.0, 1.0], dtype=torch.float32).to(DEV)
    data = AC.Carved(torch.arange(16, dtype=torch.float32), DEV)
    tab = (_abi.InvrAdamTensor * n)()
    for i, e in enumerate(tab):
        e.param = e.grad = e.exp_avg = e.exp_avg_sq = data.ptr
        e.numel, e.lr, e.weight_decay, e.bc1, e.bc2_sqrt = 16 - i % 5, 5e-4 * (1 + i), 0.01 * (i % 3), 0.25 + i, -3.0
        e.active = (None, flags[1:2].data_ptr(), flags[0:1].data_ptr())[i % 3 if n > 2 else 0]
        e.grad_shift, e.step = i % 5, AC.ADVANCE_STEPS[(i + n) % len(AC.ADVANCE_STEPS)]
    before = bytes(tab)
    table = torch.frombuffer(bytearray(before), dtype=torch.uint8).clone().to(DEV)
    adam_advance(table, n, betas)
    after = read_table(table, n)
    size, differ, advanced, seen, after_raw = C.sizeof(_abi.InvrAdamTensor), 0, 0, set(), bytes(after)
    for i, (a, b) in enumerate(zip(tab, after)):
        raw_a, raw_b = before[i * size:(i + 1) * size], after_raw[i * size:(i + 1) * size]
        if n > 2 and i % 3 == 2:
            assert raw_a == raw_b, (i, 'an inactive entry was advanced')
            continue
        s = a.step + 1
        seen.add(a.step)
        advanced += 1
        assert b.step == s, (i, a.step, b.step)
        for name, want in zip(('bc1', 'bc2_sqrt'), AC.bias_corrections(s, betas)):
            got = getattr(b, name)
            assert 0.0 < got <= 1.0, (i, name, got)
            assert abs(got - want) <= AC.ulp32(want), (i, s, name, got, want)
            differ += got != want
        b.step, b.bc1, b.bc2_sqrt = a.step, a.bc1, a.bc2_sqrt
        assert bytes(b) == raw_a, (i, 'advance changed another field of the entry')
    if n >= 16:
        assert seen == set(AC.ADVANCE_STEPS)
    print('ADAM-ADVANCE n=%d betas=%s: %d of %d bias corrections not bit-identical to the host\'s' % (n, betas, differ, 2 * advanced))
    assert data.unchanged()


def test_adam_advance_covers_every_starting_step_in_small_tables():
    """(the tables of 1 entry start at one step each: all eight starting steps as 1-entry tables too)"""
    for s0 in AC.ADVANCE_STEPS:
        data = AC.Carved(torch.zeros(4), DEV)
        tab = (_abi.InvrAdamTensor * 1)()
        tab[0].param = tab[0].grad = tab[0].exp_avg = tab[0].exp_avg_sq = data.ptr
        tab[0].numel, tab[0].step = 4, s0
        table = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).clone().to(DEV)
        adam_advance(table, 1)
        e = read_table(table, 1)[0]
        bc1, bc2s = AC.bias_corrections(s0 + 1)
        assert e.step == s0 + 1 and abs(e.bc1 - bc1) <= AC.ulp32(bc1) and abs(e.bc2_sqrt - bc2s) <= AC.ulp32(bc2s), (s0, e.step, e.bc1, e.bc2_sqrt)


# ---- 7. {advance, step} replayed -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [1, 2, 5])
def test_adam_advance_and_step_replayed(k):
    """The training loop's iteration — a fresh gradient written into the same buffer, invr_adam_advance, invr_adam_step on the table
    uploaded once — k times: every step is one step of the reference fed the kernel's own previous outputs and the bias corrections
    the device table holds (which test_adam_advance pins), so the rule applies step by step without an accumulated tolerance."""
    specs = [('first', 4099, 0, 0.0, 0), ('training', 16385, 8, 0.01, 0), ('training', 1025 * 16, 999, 0.0, 4), ('first', 3 * 2, 0, 0.0, 1)]
    tens = []
    for i, (kind, n, s0, wd, shift) in enumerate(specs):
        sc = AC.scalars(5e-4, wd, s0 + 1, BETAS, EPS)
        p, g, m, v = AC.make_inputs(kind, n, sc, seed=20 + i, n_grad=n >> shift)
        tens.append(Ten(p, torch.zeros_like(g), m, v, 5e-4, wd, s0, shift))
    table = upload_table(tens)                                     # bc1 / bc2_sqrt of step s0: stale until the first advance
    ct, ci = chunk_lists(tens)
    state = [{'p': t.host[0], 'm': t.host[2], 'v': t.host[3]} for t in tens]
    gen = torch.Generator().manual_seed(77)
    for it in range(k):
        grads = [1e-3 * torch.randn(t.g.n, generator=gen) for t in tens]
        for t, g in zip(tens, grads):
            t.g.t.copy_(g)
            t.g.before = t.g.bits()
        adam_advance(table, len(tens))
        adam_step(table, ct, ci)
        tab = read_table(table, len(tens))
        for i, (t, g, e) in enumerate(zip(tens, grads, tab)):
            assert e.step == specs[i][2] + it + 1
            want = AC.bias_corrections(e.step)
            assert abs(e.bc1 - want[0]) <= AC.ulp32(want[0]) and abs(e.bc2_sqrt - want[1]) <= AC.ulp32(want[1])
            t.set_step(5e-4, specs[i][3], e.step, bc=(e.bc1, e.bc2_sqrt))
            t.fences_hold((it, i))
            out = t.out()
            AC.accept('replay-k%d-it%d-%d' % (k, it, i), out, t.reference(state[i], g), family='replay')
            state[i] = out


# ---- 8. argument handling that never reaches the device ---------------------------------------------------------------------------------------
def test_adam_entry_points_check_their_arguments_on_the_host():
    L = _abi.lib()
    sc = AC.scalars(5e-4, 0.0, 3)
    t = Ten(*AC.make_inputs('training', 100, sc), step=3)
    table = upload_table([t])
    table_before = bytes(table.cpu().numpy())
    ct = torch.zeros(1, dtype=torch.int32).to(DEV)
    tp, cp, null, st = C.c_void_p(table.data_ptr()), _abi.ptr(ct, torch.int32), C.c_void_p(0), _abi.stream_ptr()
    assert L.invr_adam_step(tp, cp, cp, 0, 0.9, 0.999, EPS, st) == 0                    # nothing to do: nothing written
    assert L.invr_adam_step(null, null, null, 0, 0.9, 0.999, EPS, st) == 0
    assert L.invr_adam_advance(tp, 0, 0.9, 0.999, st) == 0
    assert L.invr_adam_advance(null, 0, 0.9, 0.999, st) == 0
    sync()
    assert t.untouched() and t.g.unchanged() and bytes(table.cpu().numpy()) == table_before
    for call, name in ((lambda: L.invr_adam_step(null, cp, cp, 1, 0.9, 0.999, EPS, st), 'invr_adam_step'),
                       (lambda: L.invr_adam_step(tp, null, cp, 1, 0.9, 0.999, EPS, st), 'invr_adam_step'),
                       (lambda: L.invr_adam_step(tp, cp, null, 1, 0.9, 0.999, EPS, st), 'invr_adam_step'),
                       (lambda: L.invr_adam_step(tp, cp, cp, -1, 0.9, 0.999, EPS, st), 'invr_adam_step'),
                       (lambda: L.invr_adam_step(tp, cp, cp, 1 << 31, 0.9, 0.999, EPS, st), 'invr_adam_step'),
                       (lambda: L.invr_adam_advance(null, 1, 0.9, 0.999, st), 'invr_adam_advance')):
        assert call() != 0
        assert name in L.invr_last_error().decode(), L.invr_last_error()
    sync()
    assert t.untouched() and t.g.unchanged() and bytes(table.cpu().numpy()) == table_before


# ---- 9. / 10. FusedAdam: the host logic around the kernel -----------------------------------------------------------------------------------
TRAJ_SHAPES = [(64, 19), (17, 64), (64, 70), (3, 64), (32, 32), (3, 32), (4099, 16), (1027,)]     # (the last one: a misaligned view)


def test_fused_adam_trajectory_as_close_to_float64_as_torch_fp32():
    """40 steps over 8 tensors (one a misaligned view t[1:]), tensors without gradient in some steps, a per-group lr change at step
    20, one group with weight decay: per tensor and for p, exp_avg, exp_avg_sq
        max |mine - exact| <= 4 max |torch fp32 - exact| + 2^-24 max |x|
    exact = torch.optim.Adam in float64 on the CPU, torch fp32 = the same in float32 (foreach=False).  (The smallest tensor has 96
    elements: a maximum over fewer would make the torch-fp32 side of the inequality a matter of luck.)"""
    from invr.optim import FusedAdam
    gen = torch.Generator().manual_seed(31)
    init = [0.1 * torch.randn(s, generator=gen) for s in TRAJ_SHAPES]
    holder = torch.zeros(TRAJ_SHAPES[-1][0] + 1).to(DEV)
    mine_p = [x.clone().to(DEV).requires_grad_() for x in init[:-1]]
    holder[1:] = init[-1].to(DEV)
    mine_p.append(holder[1:].detach().requires_grad_())
    assert mine_p[-1].data_ptr() % 16 == 4 and mine_p[-1].is_contiguous()
    p32 = [x.clone().requires_grad_() for x in init]
    p64 = [x.double().requires_grad_() for x in init]
    mk = lambda ps: [{'params': [p], 'lr': 5e-4 * (1 + k % 3), 'weight_decay': 0.01 if k == 2 else 0.0} for k, p in enumerate(ps)]
    mine = FusedAdam(mk(mine_p), 5e-4, eps=EPS)
    t32 = torch.optim.Adam(mk(p32), 5e-4, eps=EPS, foreach=False)
    t64 = torch.optim.Adam(mk(p64), 5e-4, eps=EPS, foreach=False)
    taken = [0] * len(init)
    for it in range(40):
        for k in range(len(init)):
            if (it + 3 * k) % 7 == 6:                              # no gradient for this tensor in this step
                mine_p[k].grad = p32[k].grad = p64[k].grad = None
                continue
            g = (torch.randn(init[k].shape, generator=gen) * 10.0 ** ((k % 3) - 3)).float()
            mine_p[k].grad, p32[k].grad, p64[k].grad = g.to(DEV), g.clone(), g.double()
            taken[k] += 1
        if it == 20:
            for opt in (mine, t32, t64):
                for k, grp in enumerate(opt.param_groups):
                    grp['lr'] *= 0.5 if k % 2 else 0.25
        mine.step(); t32.step(); t64.step()
    sd = mine.state_dict()['state']
    assert holder[0] == 0                                          # the float in front of the misaligned view
    for k in range(len(init)):
        assert float(sd[k]['step']) == taken[k] == float(t64.state[p64[k]]['step'])
        for name, a, b, c in (('p', mine_p[k], p32[k], p64[k]),
                              ('exp_avg', sd[k]['exp_avg'], t32.state[p32[k]]['exp_avg'], t64.state[p64[k]]['exp_avg']),
                              ('exp_avg_sq', sd[k]['exp_avg_sq'], t32.state[p32[k]]['exp_avg_sq'], t64.state[p64[k]]['exp_avg_sq'])):
            exact = c.detach()
            e_mine = float((a.detach().cpu().double() - exact).abs().max())
            e_t32 = float((b.detach().double() - exact).abs().max())
            slack = 2.0 ** -24 * float(exact.abs().max())
            print('ADAM-TRAJ tensor %d %s %s: |mine - exact| = %.3e, |torch32 - exact| = %.3e, ratio %.3f'
                  % (k, tuple(init[k].shape), name, e_mine, e_t32, e_mine / max(e_t32, 1e-300)))
            assert e_mine <= 4 * e_t32 + slack, (k, name, e_mine, e_t32)


def test_fused_adam_builds_its_table_once_and_carries_the_steps_over():
    """Gradients written in place, lr unchanged: one device table for all steps, step counts on the device; an lr change or a moved
    gradient rebuilds it with the step counts so far."""
    from invr.optim import FusedAdam
    gen = torch.Generator().manual_seed(32)
    ps = [(0.1 * torch.randn(s, generator=gen)).to(DEV).requires_grad_() for s in [(64, 19), (3,), (16385,)]]
    for p in ps:
        p.grad = torch.zeros_like(p)
    opt = FusedAdam([{'params': [p], 'lr': 5e-4, 'weight_decay': 0.0} for p in ps], 5e-4, eps=EPS)
    steps_of = lambda: [read_table(opt._table, len(ps))[i].step for i in range(len(ps))]
    for it in range(5):
        for p in ps:
            p.grad.copy_(1e-3 * torch.randn(p.shape, generator=gen))
        opt.step()
        if it == 0:
            table_ptr, key = opt._table.data_ptr(), opt._plan_key
    assert opt._table.data_ptr() == table_ptr and opt._plan_key == key and opt._pending == 5
    sync()
    assert steps_of() == [5, 5, 5]
    sd = opt.state_dict()
    assert [float(sd['state'][i]['step']) for i in range(3)] == [5.0, 5.0, 5.0] and opt._pending == 0
    opt.param_groups[1]['lr'] = 1e-4                               # a scheduler writes group['lr']
    opt.step()
    assert opt._plan_key != key
    sync()
    tab = read_table(opt._table, 3)
    assert steps_of() == [6, 6, 6] and tab[1].lr == AC.f32(1e-4) and tab[0].lr == AC.f32(5e-4)
    key = opt._plan_key
    ps[0].grad = ps[0].grad.clone()                                # the gradient moved
    ps[1].grad = None                                              # ... and one tensor has none this step
    opt.step()
    assert opt._plan_key != key and len(opt._plan_params) == 2
    sync()
    tab = read_table(opt._table, 2)
    assert [tab[0].step, tab[1].step] == [7, 7] and tab[0].param == ps[0].data_ptr() and tab[1].param == ps[2].data_ptr()
    for e in tab:
        bc1, bc2s = AC.bias_corrections(7)
        assert abs(e.bc1 - bc1) <= AC.ulp32(bc1) and abs(e.bc2_sqrt - bc2s) <= AC.ulp32(bc2s)
    sd = opt.state_dict()
    assert [float(sd['state'][i]['step']) for i in range(3)] == [7.0, 6.0, 7.0]


# ---- 11. the gradient arena's row-scalar gradients through FusedAdam.attach ----------------------------------------------------------------------
def test_fused_adam_arena_row_gradients_step_the_tables_as_dense_gradients_do(small_setup):
    """FusedAdam.attach(net): row gradients written by hand into Embedder.row_grad() (row_grad_dirty set) step the part tables exactly as
    the dense gradient row[:, None].expand(-1, F) does through a plain FusedAdam — bit-identical tables and moments, two steps."""
    import copy
    from invr.network import Network
    from invr.optim import FusedAdam
    cfg, sd, _, _ = small_setup
    net_a = Network(cfg=cfg)
    net_a.load_state_dict(sd, strict=True)
    net_a = net_a.to(DEV)
    net_b = copy.deepcopy(net_a)
    mk = lambda net: [{'params': [p], 'lr': 5e-4, 'weight_decay': 0.0} for p in net.parameters() if p.requires_grad]
    opt_a = FusedAdam(mk(net_a), 5e-4, eps=EPS).attach(net_a)
    opt_b = FusedAdam(mk(net_b), 5e-4, eps=EPS)
    gen = torch.Generator().manual_seed(41)
    emb = lambda net: [pn.embedder for pn in net.tpose_human.part_networks]
    tables = lambda e: ([e.dense] if e.separate_dense else []) + [e.hash]
    for it in range(2):
        for ea, eb in zip(emb(net_a), emb(net_b)):
            rg = ea.row_grad()
            row = (1e-3 * torch.randn(rg.numel(), generator=gen)).to(DEV)
            row[::3] = 0.0                                            # rows no sample reached
            rg.copy_(row)
            ea.row_grad_dirty = True
            o = 0
            for t in tables(eb):
                rows = t.numel() // eb.f
                t.grad = row[o:o + rows, None].expand(-1, eb.f).reshape(t.shape).contiguous()
                o += rows
            assert o == rg.numel()
        opt_a.step()
        opt_b.step()
        shift = int(emb(net_a)[0].f).bit_length() - 1
        assert shift >= 2 and {e.grad_shift for e in read_table(opt_a._table, len(opt_a._plan_params))} == {shift}
        assert {e.grad_shift for e in read_table(opt_b._table, len(opt_b._plan_params))} == {0}
    sync()
    n = 0
    for ea, eb in zip(emb(net_a), emb(net_b)):
        for ta, tb in zip(tables(ea), tables(eb)):
            assert AC.same_bits(ta, tb) and not AC.same_bits(ta, sd_table(sd, ta, net_a))
            for k in ('exp_avg', 'exp_avg_sq'):
                assert AC.same_bits(opt_a.state[ta][k], opt_b.state[tb][k]), k
            n += 1
    assert n >= 5 and len(opt_a._plan_params) == n == len(opt_b._plan_params)
    assert [float(s['step']) for s in opt_a.state_dict()['state'].values()] == [2.0] * n


def sd_table(sd, t, net):
    """the initial value of table parameter `t` of `net` in the state dict it was loaded from"""
    name = next(k for k, p in net.named_parameters() if p is t)
    return sd[name]
