"""CPU: the bodies of tests/test_gpu_perceptual.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — every stored layer of the perceptual loss's forward and backward against float64 and every discrete rule
exactly, without a GPU.  Every shape up to 33 x 16 runs in the default CPU suite; the production sizes 56 x 56 and 64 x 64 only under
HOSTSIM_FULL=1.  What the device adds — the hardware's MFMA instead of its restatement, concurrent workgroups — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_perceptual as M
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


PER_CASE = ('test_forward_layers', 'test_backward_layers', 'test_means_and_out8', 'test_end_to_end')


def _over(body, cases):
    @pytest.mark.parametrize('case', cases)
    def test(case):
        body(case)
    return test


for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n in PER_CASE and not os.environ.get('HOSTSIM_FULL'):
        globals()['test_hostsim__' + _n[5:]] = _over(getattr(M, _n), M.SMALL)
    else:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
