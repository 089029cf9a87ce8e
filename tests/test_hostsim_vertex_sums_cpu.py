"""CPU: the bodies of tests/test_gpu_vertex_sums.py on the wave machine (tests/hostsim: the kernel SOURCES compiled for the host and
executed wave by wave) — the builder of the de-hashed vertex tables entry by entry, and the encoder with the tables on against the
tables off, without a GPU.  The `all` cap is 2^17 vertices per level here (levels up to res 50; 2^24 — 25 M table entries through the
wave machine — only under HOSTSIM_FULL=1); what the device adds, the levels up to res 251 among it, is left to -m gpu."""
import os

import pytest

import tests.test_gpu_vertex_sums as V
from tests.hostsim import harness

FULL = bool(os.environ.get('HOSTSIM_FULL'))


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    old = V.DEV, V.ALL
    V.DEV, V.ALL = 'cpu', (V.ALL if FULL else 2 ** 17)
    V.base_grid.cache_clear(); V.vertex_grid.cache_clear()
    try:
        with harness.activate() as counters:
            yield counters
            assert counters.anomalies == 0, counters.anomalies
    finally:
        V.DEV, V.ALL = old
        V.base_grid.cache_clear(); V.vertex_grid.cache_clear()


@pytest.mark.parametrize('tag,capname', V.BUILD, ids=['%s-%s' % c for c in V.BUILD])
def test_hostsim__vertex_sums_builder(tag, capname):
    V.test_vertex_sums_builder(tag, capname)


@pytest.mark.parametrize('tag,kind,n', V.ENC, ids=['%s-%s-%d' % c for c in V.ENC])
def test_hostsim__vertex_sums_encoder(tag, kind, n):
    V.run_encoder_case(tag, kind, n)


test_hostsim__vertex_sums_cap_zero_is_off = V.test_vertex_sums_cap_zero_is_off
test_hostsim__ties_cloud_reaches_the_far_corner_of_a_moved_level = V.test_ties_cloud_reaches_the_far_corner_of_a_moved_level
test_hostsim__vertex_sums_five_parts_one_launch = V.test_vertex_sums_five_parts_one_launch
