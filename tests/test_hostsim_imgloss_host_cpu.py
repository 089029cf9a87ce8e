"""CPU: the bodies of tests/test_gpu_imgloss_host.py on the wave machine (tests/hostsim).  The training iterations on the golden
64 x 64 scene (several renders with their backward per term) run only under HOSTSIM_FULL=1; the kernels themselves are covered by
tests/test_hostsim_imgloss_cpu.py in the default CPU suite."""
import os

import pytest

import tests.test_gpu_imgloss_host as M
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV
    M.DEV = 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M.DEV = old


step = M.step
if os.environ.get('HOSTSIM_FULL'):
    for _n in [n for n in dir(M) if n.startswith('test_')]:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
