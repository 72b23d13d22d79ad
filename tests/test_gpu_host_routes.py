"""The route of the host-buffer entries on the GPU (tests/host_route_checks.py): the same cases as on the interpreter, here with the copy streams
and the two compute streams really running side by side."""
import pytest

import host_route_checks as hc
from global_racetrajectory_optimization_amd import engine


@pytest.fixture()
def eng():
    e = engine.Engine(0)
    yield e
    e.close()


@pytest.mark.gpu
def test_warm_start_through_the_host_entries(eng, monkeypatch):
    hc.check_warm_start_through_the_host_entries(eng, monkeypatch)


@pytest.mark.gpu
def test_span_counts_calls(eng, monkeypatch):
    hc.check_span_counts_calls(eng, monkeypatch)
