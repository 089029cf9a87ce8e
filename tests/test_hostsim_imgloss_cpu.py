"""CPU: the bodies of tests/test_gpu_imgloss.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and executed
wave by wave) — the SSIM and TV terms' stored maps, values and gradients against float64, the objective's twins bit for bit, without a
GPU.  What the device adds — its own fused multiply-add and division, concurrent workgroups — is left to -m gpu."""
import pytest

import tests.test_gpu_imgloss as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV
    M.DEV = 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.DEV = old


for _n in [n for n in dir(M) if n.startswith('test_')]:
    globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
