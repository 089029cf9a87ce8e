"""CPU: the layer-local and exact-property bodies of tests/test_gpu_lpips.py on the wave machine (tests/hostsim: the kernel SOURCES
compiled for the host and executed wave by wave) at 16 x 16 (relu5_3 is 1 x 1: every strip shape from 16 x 1 to 1 x 16) and 17 x 19
(odd in front of every pool, partial tiles, two tile columns).  What the device adds — the hardware's MFMA instead of its restatement,
concurrent workgroups, the larger shapes — is left to -m gpu."""
import pytest

import tests.test_gpu_lpips as M
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


CASES = ['16x16-rand-0.05', '17x19-rand-0.002']          # every body, layer-local and exact-property, at both shapes


def _over(body, cases):
    @pytest.mark.parametrize('case', cases)
    def test(case):
        body(case)
    return test


for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n == 'test_argument_checks_launch_nothing':
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
    else:
        globals()['test_hostsim__' + _n[5:]] = _over(getattr(M, _n), CASES)
