"""CPU: the bodies of tests/test_gpu_tracked_raw.py at 64 x 64 on the wave machine (tests/hostsim: the kernel SOURCES compiled for the
host and executed wave by wave) — invr_render_fwd_tracked against the untracked call bit for bit, the dirty-bit contract over the
whole buffer, and the frames' own preconditions (a row dirty only from the frame before, an empty word, an empty ray, a ray with an
empty and a live pass), without a GPU.  What the device adds — the nontemporal stores, frames in flight — is left to -m gpu."""
import pytest

import tests.test_gpu_tracked_raw as T
from tests.hostsim import harness


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old, T.DEV = T.DEV, 'cpu'
    try:
        with harness.activate() as counters:
            yield counters
            # no kernel read a lane that was not taking part in the operation (readlane / shuffle from a disabled lane)
            assert counters.anomalies == 0, counters.anomalies
    finally:
        T.DEV = old


SAMPLES = T.FAST + T.FALLBACK
test_hostsim__tracked_entry_refuses_occ_weights_and_a_short_buffer = T.test_tracked_entry_refuses_occ_weights_and_a_short_buffer


@pytest.mark.parametrize('S', SAMPLES + (T.RAY_MAJOR,))
def test_hostsim__sequence_of_three_poses_into_one_pair(S):
    T.body_sequence(S, 64)


@pytest.mark.parametrize('S', SAMPLES)
def test_hostsim__poisoned_start(S):
    T.body_poisoned(S, 64)


@pytest.mark.parametrize('S', SAMPLES)
def test_hostsim__undersized_max_active(S):
    T.body_undersized(S, 64)


@pytest.mark.parametrize('S', SAMPLES)
def test_hostsim__empty_frame_cleans_the_buffer(S):
    T.body_empty(S, 64)


@pytest.mark.parametrize('S', T.FAST)
def test_hostsim__random_bg_epsilon_computes_the_empty_passes(S):
    T.body_random_bg(S, 64)
