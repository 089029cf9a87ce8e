"""CPU: the bodies of tests/test_gpu_merge_modes.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the part merge and its transpose per survivor in every merge mode, without a GPU.  By default frame A is cut
down to the 640 rays [2000, 2640) of the frame (trimmed like the whole one: still more than one slot group, B its first 256 rays)
and the census of the whole frame is left out; HOSTSIM_FULL=1 runs the whole frame A and the census.  What the device adds — float
atomics from concurrent workgroups, the hardware's division and square root — is left to -m gpu."""
import os

import pytest

import tests.test_gpu_merge_modes as M
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = M.DEV, M.A_RAYS
    M.DEV = 'cpu'
    M.A_RAYS = None if FULL else (2000, 2640)
    M._frames.clear()
    M._batches.clear()
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        M._frames.clear()
        M._batches.clear()
        M.DEV, M.A_RAYS = old


LEFT_OUT = set() if FULL else {'test_frame_a_holds_every_class'}
for _n in [n for n in dir(M) if n.startswith('test_')]:
    if _n not in LEFT_OUT:
        globals()['test_hostsim__' + _n[5:]] = getattr(M, _n)
small_net = M.small_net
