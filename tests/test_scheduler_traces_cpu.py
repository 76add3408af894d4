"""ContinuousBatcher replays the scenarios of tests/scheduler_scenarios.py on the scripted engine and must reproduce the records of
tests/golden/scheduler_traces.json (written by `python -m tests.scheduler_scenarios <commit>` on a checkout of the commit its first
key names): the same engine calls in the same order, the same events of every step, the same stats, errors and side tables, the
same pool at the end."""
import json

import pytest

from tests import scheduler_scenarios as sc


@pytest.fixture(scope="module")
def golden():
    with open(sc.GOLDEN) as f:
        doc = json.load(f)
    assert next(iter(doc)) == "generated_from_commit" and len(doc["generated_from_commit"]) == 40
    return doc["scenarios"]


def _first_difference(name, key, want, got):
    if isinstance(want, list) and isinstance(got, list):
        for i, (w, g) in enumerate(zip(want, got)):
            if w != g:
                return f"{name}: {key}[{i}] is {g!r}, recorded {w!r} (after {got[max(i - 3, 0):i]!r})"
        return f"{name}: {key} has {len(got)} items, recorded {len(want)}; the longer one goes on with {max(want, got, key=len)[min(len(want), len(got))]!r}"
    if isinstance(want, dict) and isinstance(got, dict):
        for k in sorted(set(want) | set(got)):
            if want.get(k) != got.get(k):
                return f"{name}: {key}[{k!r}] is {got.get(k)!r}, recorded {want.get(k)!r}"
    return f"{name}: {key} is {got!r}, recorded {want!r}"


def test_every_scenario_is_recorded(golden):
    assert sorted(golden) == sorted(sc.NAMES)


@pytest.mark.parametrize("name", sc.NAMES)
def test_scenario_replays_its_recorded_trace(golden, name):
    want, got = golden[name], sc.play(name)
    assert sorted(got) == sorted(want), name
    for key in want:
        assert got[key] == want[key], _first_difference(name, key, want[key], got[key])
