"""CPU: the bodies of tests/test_gpu_knn_adversarial.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the brute-force KNN against the exact integer reference, k_knn_pairs against brute force on the degenerate
vertex sets of tests/knn_cases.py, one workspace reused across scenes — with a reduced size table: a few hundred rays per frame, least
counts of 20.  Which side of the front plan's N >= 4 * cells switch a run is on is only asserted by -m gpu (a frame of 4 samples per
lattice cell takes the wave machine a minute; tests/test_hostsim_production_cpu.py has one); the coarse lattices' 665 cells put
their runs on the masked side here too.  HOSTSIM_FULL=1 runs every run of every scene at the GPU module's own sizes and asserts the sides."""
import os

import pytest

import tests.test_gpu_knn_adversarial as A
from tests import knn_cases as K
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))

RUNS = {
    'full64': dict(rays=320, S=64, thresh=0.05),
    's16': dict(rays=512, S=16, thresh=0.05),
    'jit30': dict(rays=96, S=30, thresh=0.1, all_survive=True, jitter=True),
    'two': dict(rays=768, S=2, thresh=0.1, all_survive=True),
    'class_off': dict(rays=128, S=16, thresh=0.45),
    'tiny': dict(rays=128, S=16, thresh=1e-3, all_survive=True),
    'render64': dict(rays=192, S=64, thresh=0.05, mode='render'),
    's30': dict(rays=256, S=30, thresh=0.05),
    'jit30ge': dict(rays=160, S=30, thresh=0.05, jitter=True),
    'pts_ge': dict(rays=16384, S=1, thresh=0.05, mode='points'),
    'pts_lt': dict(rays=2048, S=1, thresh=0.1, all_survive=True, mode='points'),
}
MINC = 20
if FULL:                       # the GPU module's own frames (2 - 7 s each here), sides of the front-plan switch asserted
    RUNS, MINC = A.RUNS, A.MINC
A_N = A.A_N

# default suite: every scene once per cull style (thresholded lattice / everything survives) and as a point frame of one sample, the
# edges_c thresholds, one render
DEFAULT_RUNS = ('full64', 'jit30', 'pts_lt')
PAIR_CASES = [c for c in A.PAIR_CASES if FULL or c[1] in DEFAULT_RUNS or c in (('edges_c', 'class_off'), ('edges_c', 'tiny'), ('carve_spill', 'render64'),
                                                                                ('lattice', 'two'), ('edges_b', 's16'), ('coarse_tight', 's30'), ('edges_b', 'jit30ge'),
                                                                                ('edges_c', 'pts_ge'), ('lattice', 'pts_ge'), ('coarse_tight', 'pts_ge'), ('carve_spill', 'pts_ge'))]
DENSE_CASES = [(t, n) for t in A.A_SCENES for n in A_N]


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = {k: getattr(A, k) for k in ('DEV', 'RUNS', 'MINC', 'A_N', 'ASSERT_SIDES')}
    A.DEV, A.RUNS, A.MINC, A.A_N, A.ASSERT_SIDES = 'cpu', RUNS, MINC, A_N, FULL
    A.a_case.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            assert counters.anomalies == 0, counters.anomalies
    finally:
        for k, v in old.items():
            setattr(A, k, v)
        A.a_case.cache_clear()


@pytest.fixture(scope='module')
def small_net(hostsim):
    import copy
    import torch
    from invr.config import make_cfg
    from invr.network import Network
    torch.manual_seed(11)
    cfg = make_cfg(table_log2=12)
    return cfg, Network(cfg=copy.deepcopy(cfg)).eval()


@pytest.mark.parametrize('tag,n', DENSE_CASES, ids=A.ids(DENSE_CASES))
def test_hostsim__dense_knn_vs_exact_reference(tag, n):
    A.run_dense_case(tag, n)


test_hostsim__exact_reference_has_ties_on_the_list_boundary = A.test_exact_reference_has_ties_on_the_list_boundary


@pytest.mark.parametrize('name,run', PAIR_CASES, ids=A.ids(PAIR_CASES))
def test_hostsim__knn_pairs_vs_brute_force(small_net, name, run):
    A.test_knn_pairs_vs_brute_force(small_net, name, run)


def test_hostsim__workspace_reused_across_scenes(small_net):
    A.test_workspace_reused_across_scenes(small_net)


def test_hostsim__one_sample_per_ray_is_refused(small_net):
    A.test_one_sample_per_ray_is_refused(small_net)


def test_scene_builders_meet_their_specification():
    """tests/knn_cases.py, no kernel involved: part lengths and padded LDS slot totals of the edge scenes, the dyadic scenes ARE on the
    lattice, the integer reference against a float64 brute force on a sample, ties ordered by row."""
    import numpy as np
    want = {'edges_a': 4416, 'edges_b': 4416, 'edges_c': 7488, 'carve_fit': 7680, 'carve_spill': 7744}
    for name, slots in want.items():
        b = K.build(name)
        assert tuple(b['lengths2'][0]) == K.EDGES[name] and K.padded_slots(b['lengths2'][0]) == slots
        assert (slots > K.LDS_SLOTS) == (name == 'carve_spill')
    fit, spill = K.build('carve_fit'), K.build('carve_spill')
    assert np.array_equal(fit['part_pts'][0, :, :1536], spill['part_pts'][0, :, :1536])            # same vertices apart from the one extra
    b = K.lattice()
    L = b['lengths2'][0]
    q = K.query_block((-6, 0, -4), (6, 14, 4), n=64)
    rows, d2 = K.exact_knn(q, b['part_pts'][0], L, 5)
    for p in range(5):
        v = b['part_pts'][0, p, :L[p]].astype(np.float64)
        ext = v.max(0) - v.min(0)
        assert int((ext == 0).sum()) == (0, 0, 1, 2, 3)[p]                                          # shells, plate, line, point
        dd = ((q[:, None, :].astype(np.float64) - v[None]) ** 2).sum(-1)
        order = np.lexsort((np.broadcast_to(np.arange(L[p]), dd.shape), dd), axis=1)[:, :5]
        assert np.array_equal(order, rows[:, p]) and np.array_equal(np.take_along_axis(dd, order, 1), d2[:, p])
    # a tie is decided by the row
    tie = d2[..., 3] == d2[..., 4]
    assert tie.any() and bool((rows[..., 3][tie] < rows[..., 4][tie]).all())
    o = K.offset()
    e = K.build('edges_c')
    assert np.abs(o['part_pts'][0, 1, :4097] - e['part_pts'][0, 1, :4097] - np.array([8.0, -8.0, 8.0])).max() < 1e-6
