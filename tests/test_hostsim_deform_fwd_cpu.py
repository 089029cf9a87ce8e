"""CPU: the bodies of tests/test_gpu_deform_fwd.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — k_deform_points, k_warp_dense and the three instantiations of k_deform_pairs element by element against the
float64 reference, and the per-frame slice table entry by entry, without a GPU.  Every case runs in the default CPU suite except the UV
volume padded past 2^24 elements (a 70 MB volume and its float64 copy), which runs under HOSTSIM_FULL=1.  What the device adds — the
hardware's exp2 / log2 / rcp pipes and its tanhf instead of libm, the matrix cores' accumulation order — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_deform_fwd as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.set_device('cpu')
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.set_device(old)


LARGE = set() if os.environ.get('HOSTSIM_FULL') else {'test_pair_deformer_big_volume'}
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n not in LARGE:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
