"""The route of the host-buffer entries on the SIMT interpreter (tests/host_route_checks.py): the interpreter's streams are synchronous, so what
is checked here is the choice of the route -- a warm start that applies takes the one launch and is honoured -- and the bookkeeping of a span."""
import pytest

import host_route_checks as hc
from global_racetrajectory_optimization_amd import engine


@pytest.fixture()
def eng(emu_lib):
    e = engine.Engine(0, lib_path=emu_lib)
    yield e
    e.close()


def test_warm_start_through_the_host_entries(eng, monkeypatch):
    hc.check_warm_start_through_the_host_entries(eng, monkeypatch)


def test_span_counts_calls(eng, monkeypatch):
    hc.check_span_counts_calls(eng, monkeypatch)
