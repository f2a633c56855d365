"""Which kernels a generator forward launches, in which order and with which arguments, for every calling context and
switch setting of tests/route_spy.py -- held to the tables recorded under tests/golden/.  The routing of
utils/stylegan2/models.py is policy, not arithmetic: a route that moves shows up HERE, where the mistake was made, and
not as a launch more or a hand-over less somewhere in a profile."""
import os

import pytest

from tests import route_spy
from tests.conftest import GOLDEN


def _check(monkeypatch, golden, size, device, sizes):
    want = route_spy.load(os.path.join(GOLDEN, golden))
    assert sorted(want) == sorted(route_spy.keys(sizes))             # every configuration is recorded, none left out
    mine = [k for k in route_spy.keys((size,))]
    got = route_spy.record_size(monkeypatch, size, device)
    assert sorted(got) == sorted(mine)
    for key in mine:
        assert got[key] == want[key], key


@pytest.mark.parametrize('size', route_spy.CPU_SIZES)
def test_routes_of_the_emulated_path_are_the_recorded_ones(monkeypatch, size):
    _check(monkeypatch, 'routes_cpu.json', size, 'cpu', route_spy.CPU_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize('size', route_spy.GPU_SIZES)
def test_routes_on_the_device_are_the_recorded_ones(monkeypatch, size):
    """The real wrappers: the ToRGB partial sums, the strips on the auxiliary stream, the prefetch and the fused last
    layer exist only with a device stream."""
    _check(monkeypatch, 'routes_gpu.json', size, 'cuda', route_spy.GPU_SIZES)
