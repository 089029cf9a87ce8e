"""CPU: the bodies of tests/test_gpu_mesh.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and executed
wave by wave, one workgroup after another) — the masks, counts, prefix sums, vertices and triangles of the surface extraction against
the contract, without a GPU.  The 33 x 16 x 65 case runs only under HOSTSIM_FULL=1.  What the device adds — concurrent workgroups,
graph replay — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_mesh as M
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


def _over(body, cases):
    @pytest.mark.parametrize('case', cases)
    def test(case):
        body(case)
    return test


for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n == 'test_mesh_against_the_contract' and not os.environ.get('HOSTSIM_FULL'):
        globals()['test_hostsim__' + _n[5:]] = _over(getattr(M, _n), M.SMALL)
    else:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
