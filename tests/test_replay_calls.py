"""DeviceTrainer.replay() on host stand-ins (tests/replay_standin.py): every call it issues on the batch - name, scalar
arguments, pointers as (buffer, byte offset) -, what it returns and the counters after each replay, against
tests/golden/replay_calls.json.  The fixture was recorded by tests/record_replay_calls.py from the commit before the
replay bodies became one step; it pins the issue order of every sampling and fit mode without a GPU."""
import json
import os

import pytest

from tests import replay_standin as st

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "replay_calls.json")
CASES = st.cases()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases(golden):
    assert sorted(golden) == sorted(c[0] for c in CASES) and len(golden) == len(CASES)
    assert all(len(c[3]) >= 3 for c in CASES)                 # start, draws, beta() and the target_sync period move


@pytest.mark.parametrize("name,kw,hook,sched,batch_size", CASES, ids=[c[0] for c in CASES])
def test_replay_issues_the_recorded_calls(monkeypatch, golden, name, kw, hook, sched, batch_size):
    import ofighters_amd.trainer as tr
    got = json.loads(json.dumps(st.run_case(tr, monkeypatch.setattr, kw, hook, sched, batch_size)))
    want = golden[name]
    assert got["setup"] == want["setup"]
    assert len(got["replays"]) == len(want["replays"])
    for i, (g, w) in enumerate(zip(got["replays"], want["replays"])):
        assert g["log"] == w["log"], "replay %d" % i         # entry for entry
        assert g["returned"] == w["returned"], "replay %d" % i
        assert g["state"] == w["state"], "replay %d" % i     # fit_steps, draws, losses, grad_norms, scratch sizes
