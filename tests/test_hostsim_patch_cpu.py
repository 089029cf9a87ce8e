"""CPU: the bodies of tests/test_gpu_patch.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and executed
wave by wave) — the ordered compaction of k_patch_batch (ballots, lane ranks, the wave totals in LDS, the base carried from round to
round), its rays and its gathers against the contract and the reference's recorded outputs, without a GPU.  The 256 x 256 window (64
rounds) runs only under HOSTSIM_FULL=1."""
import os

import pytest

import tests.test_gpu_patch as M
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
    @pytest.mark.parametrize('case', cases, ids=lambda w: '%s_%dx%d' % w)
    def test(case):
        body(case)
    return test


for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n == 'test_patch_against_the_contract' and not os.environ.get('HOSTSIM_FULL'):
        globals()['test_hostsim__' + _n[5:]] = _over(getattr(M, _n), M.SMALL)
    else:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
