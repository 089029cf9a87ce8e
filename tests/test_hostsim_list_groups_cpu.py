"""CPU: tests/test_gpu_list_groups.py through the host build of the kernel sources (tests/hostsim) — the multi-group walk of the pair
and winner lists against its own single-group case.  By default one sum flow ('mean') and one select flow that reads part_dist
('mindist'); HOSTSIM_FULL=1 runs all four merge modes."""
import os

import pytest

import tests.test_gpu_list_groups as G
from tests.hostsim import harness

AGGRS = G.AGGRS if os.environ.get('HOSTSIM_FULL') else ['mean', 'mindist']


@pytest.fixture(scope='module', autouse=True)
def hostsim():
    with harness.activate() as counters:
        yield counters
        assert counters.anomalies == 0, counters.anomalies


@pytest.fixture(scope='module')
def small_net(hostsim):
    return G.make_small_net('cpu')


@pytest.mark.parametrize('aggr', AGGRS, ids=[a or 'max' for a in AGGRS])
def test_hostsim_list_groups_whole_frame_equals_single_group_chunks(small_net, aggr):
    G.check_list_groups(*small_net, aggr, 'cpu')
