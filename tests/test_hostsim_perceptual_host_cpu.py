"""CPU: the bodies of tests/test_gpu_perceptual_host.py on the wave machine (tests/hostsim).  The packed-weight cache runs in the
default CPU suite; the training iterations on the golden 64 x 64 scene (three renders with their backward and the 64 x 64 VGG) only
under HOSTSIM_FULL=1."""
import os

import pytest

import tests.test_gpu_perceptual_host as M
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
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if os.environ.get('HOSTSIM_FULL') or _n == 'test_packed_weights_follow_an_in_place_change':
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
