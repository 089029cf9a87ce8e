"""CPU: the bodies of tests/test_gpu_eval_metrics.py on the wave machine (tests/hostsim: the kernel SOURCES of csrc/k_metrics.hip
compiled for the host and executed wave by wave) — rank-and-scatter, rectangle, uint8 image, the float64 SSE / SSIM sums and the
Evaluator around them against the float64 NumPy restatement (tests/eval_metrics_reference.py), without a GPU.  The 512 x 512 cases
run only under HOSTSIM_FULL=1 (and in -m gpu); the driver-level cases (run_evaluate(metrics='device'): renderer lanes, streams,
events) are the device's."""
import os

import numpy as np
import pytest

import tests.test_gpu_eval_metrics as G
from tests import eval_metrics_reference as R
from tests.hostsim import harness

BORROWED = [G]


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = [m.DEV for m in BORROWED]
    for m in BORROWED:
        m.DEV = 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        for m, d in zip(BORROWED, old):
            m.DEV = d


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_metrics_kernels_512'}
for _m in BORROWED:
    for _n in [n for n in dir(_m) if n.startswith('test_')]:
        if _n not in LARGE and not getattr(getattr(_m, _n), 'gpu_only', False):
            globals()['test_hostsim__' + _n[5:]] = getattr(_m, _n)


def test_hostsim_kernels_ran(hostsim):
    """the borrowed bodies did launch kernels of the host build (five per frame)"""
    hostsim.reset()
    G.check_frame(16, 16, 'ellipse', 'noise', True)
    assert hostsim.launches == 5


def test_restatement_two_formulations_agree():
    """The restatement's window form against an independent one (running sums along each axis, crop of the 3-pixel border — the shape of
    scipy.ndimage.uniform_filter + skimage's crop), and against scikit-image itself where that package can be imported (it cannot in
    this project's environment: that branch has never run here)."""
    rng = np.random.default_rng(5)
    for shape in ((40, 52), (7, 7), (97, 131)):
        a, b = rng.random(shape + (3,)), 0.9 + 1e-3 * rng.standard_normal(shape + (3,))

        def box(x):
            c = np.cumsum(np.pad(x, ((1, 0), (1, 0))), axis=0).cumsum(axis=1)
            return (c[7:, 7:] - c[:-7, 7:] - c[7:, :-7] + c[:-7, :-7]) / 49.0
        tot = []
        for ch in range(3):
            x, y = a[..., ch], b[..., ch]
            ux, uy = box(x), box(y)
            vx, vy, vxy = R.COV_NORM * (box(x * x) - ux * ux), R.COV_NORM * (box(y * y) - uy * uy), R.COV_NORM * (box(x * y) - ux * uy)
            tot.append((((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))).mean())
        assert abs(np.mean(tot) - R.ssim(a, b)) <= 1e-11          # (the running sums lose a few digits to cancellation)
        try:
            from skimage.metrics import structural_similarity
        except ImportError:
            structural_similarity = None
        if structural_similarity is not None:
            assert abs(structural_similarity(a, b, channel_axis=2, data_range=2.0) - R.ssim(a, b)) <= 1e-12
    assert R.bounding_rect(np.zeros(12, bool), 3, 4) == (0, 0, 0, 0)
    assert R.to_u8_bgr(np.array([[[-0.25, 1.0, 2.0]]]))[0, 0].tolist() == [255, 255, 0]          # B,G,R order, clamped
    assert R.to_u8_bgr(np.float32([[[0.3, 0.499, 0.7]]]))[0, 0].tolist() == [178, 127, 77]
    with pytest.raises(ValueError):
        R.ssim(np.zeros((6, 9, 3)), np.zeros((6, 9, 3)))


def test_hostsim_metrics_do_not_depend_on_lane_or_wave_order():
    """k_mask_scatter ranks through LDS wave counts, k_image_metrics hands its row sums between the waves of a workgroup through LDS:
    the kernel cases at two sizes again with the lanes in a pseudo-random order and the waves reversed (a separate process: the order
    is fixed when the library loads)."""
    import subprocess
    import sys
    env = dict(os.environ, HOSTSIM_LANE_ORDER='shuffle:7', HOSTSIM_WAVE_ORDER='reverse')
    r = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-q', '-x', '-p', 'no:cacheprovider', '-k',
                        'metrics_kernels and (64x48 or 97x131) or bit_identical'],
                       env=env, capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
