"""Per-arena episodes on the CPU: the model the GPU tests compare against (tests/autoreset_oracle.py) exercises what it
must, and TrainingRollout(auto_reset=True) makes the calls, drains the sums and refuses the arguments the way its
docstring says - against a recording stand-in for the engine, like tests/test_action_repeat.py."""
import numpy as np
import pytest

from ofighters_amd import checkpoint
from ofighters_amd.rollout import TrainingRollout
from tests import autoreset_oracle as ao
from tests.rollout_standin import FakeEngine, FakeTrainer, fake_device_buffers


# ------------------------------------------------------------------------------------------------- 1. the model
@pytest.mark.parametrize("name", ["M8", "M13"])
def test_scenario_conditions(name):
    """The conditions without which the GPU comparison would be vacuous."""
    sc = ao.run(**ao.SCENARIOS[name])
    print("%s: by death %d, by the clock %d, episodes %s, waiting %d, zero draws %d"
          % (name, sc["by_death"], sc["by_clock"], list(sc["episodes"]), sc["waiting"], sc["zero_draws"]))
    assert sc["by_death"] >= 1
    assert sc["by_clock"] >= 1
    assert sc["episodes"].max() >= 3
    assert sc["waiting"] >= 1
    assert sc["zero_draws"] >= 1
    assert sc["restarts"].sum() == sc["by_death"] + sc["by_clock"] == sc["episodes"].sum()
    last = sc["snapshots"][-1]
    assert last["sums"][0, -2] == sc["episodes"].sum()           # every restart banked one episode ...
    assert last["sums"][0, -1] + last["time"].sum() == ao.N * ao.STEPS     # ... and every lock-step belongs to one


def test_a_dead_ship_is_finished_on_the_second_call():
    """The lock-step between the two calls is the one that captures the losing frame: a death restart at lock-step t
    means the selected ships were dead already at lock-step t - 1, where the arena did not restart."""
    sc = ao.run(**ao.SCENARIOS["M8"])
    sel = list(ao.SCENARIOS["M8"]["selected"])
    seen = 0
    for t in range(1, ao.STEPS):
        for a in np.flatnonzero(sc["deaths"][t]):
            assert sc["dones"][t - 1][a, sel].all() and not sc["restarts"][t - 1][a]
            assert sc["snapshots"][t - 1]["dead_once"][a, sel].all()
            assert not sc["dones"][t][a].any() and not sc["snapshots"][t]["dead_once"][a].any()
            seen += 1
    assert seen == sc["by_death"]


def test_nothing_selected_is_the_global_clock():
    sc = ao.run(**ao.SCENARIOS["nobody"])
    assert sc["by_death"] == 0 and sc["restarts"].sum() == 10
    assert set(sc["episodes"]) <= {2, 3}
    assert (sc["restarts"][[40, 80]] == 1).all() and sc["restarts"].sum(axis=1).max() == ao.N
    assert not any(s["dead_once"].any() for s in sc["snapshots"])


# ------------------------------------------------------------------------------------------- 2. the call sequence
class _Engine(FakeEngine):
    """The stand-in with the per-arena restart; spawn, restart and sync are logged.  Every restart_finished banks one
    episode of `tick` lock-steps per arena."""
    def sync(self): self.log.append("sync")
    def spawn_random(self, seed): self.log.append("spawn")
    def restart_random(self, seed):
        self.episode += 1
        self.log.append("restart@%d" % self.tick)
    def replay_reward_source(self, ptr): self.log.append("reward_source:%r" % ptr)
    def step_repeat(self, behaviours, seed, tick0, n_ticks, hold_mask_ptr=None, actions_ptr=None, span_reward_ptr=None,
                    observe=None):
        self.log.append("step_repeat:%d:%d" % (tick0, n_ticks))
        self.tick += n_ticks
    def load_autoreset_state(self, d):
        self.log.append("autoreset_init:%s:%s" % (d["arena_episode"].shape, d["dead_once"].shape))
    def restart_finished(self, seed, ship_mask_ptr=None, max_ticks=0, seen_buf=None, group_buf=None, n_groups=1,
                         sums_buf=None):
        self.log.append("restart_finished:%r:%r:%d:%r:%r:%d:%r" % (seed, ship_mask_ptr, max_ticks, seen_buf.ptr,
                                                                  group_buf, n_groups, sums_buf.ptr))
        sums_buf.held = sums_buf.held + np.array([[1, 2, self.N, self.N * self.tick]], np.int64)


@pytest.fixture
def fake_buffers(monkeypatch):
    return fake_device_buffers(monkeypatch)


def _rollout(**kw):
    e, t = _Engine(), FakeTrainer()
    r = TrainingRollout(e, t, ["idle", "idle"], seed=3, policy_ships=(0,), collecting_steps=3, replay_every=5, **kw)
    t.clock = lambda: r.total_steps
    return e, t, r


def test_auto_reset_off_is_todays_call_sequence(fake_buffers):
    e, t, r = _rollout(episode_ticks=4, auto_reset=False)
    r.run(9)
    e2, t2, r2 = _rollout(episode_ticks=4)                       # built without the keyword
    r2.run(9)
    assert e.log == e2.log and len(e.log) > 60
    assert [l for l in e.log if l.startswith("restart")] == ["restart@4", "restart@8"]
    assert r.auto_reset is False and r2.auto_reset is False and not hasattr(r, "_auto_sums")
    assert r.length_log == [] and len(r.score_log) == 2
    assert len(fake_buffers) == 4                                # two rollouts x (mask, seen_done): no new buffer


def test_auto_reset_on_call_sequence_and_drain(fake_buffers):
    e, t, r = _rollout(episode_ticks=4, auto_reset=True)
    mask, seen, sums = r._mask.ptr, r._seen_done.ptr, r._auto_sums.ptr
    assert r._auto_sums.held.dtype == np.int64 and r._auto_sums.held.shape == (1, 4) and not r._auto_sums.held.any()
    assert e.log == ["spawn", "sync", "pin", "autoreset_init:(3,):(3, 2)"]
    del e.log[:]
    seen_uploads = r._seen_done.uploads
    call = "restart_finished:3:%r:4:%r:None:1:%r" % (mask, seen, sums)
    r.run(1)
    assert e.log == [call, "bots", "forward", "explore:0:1", "capture:0", "actions", "step", "raster"]
    r.run(3)
    assert "sync" not in e.log and r.score_log == [] and r.episode == 0
    before = len(e.log)
    r.run(1)                                                     # tick 4: the first reporting period ends
    assert e.log[before:before + 3] == [call, "sync", "bots"]
    assert r.episode == 1 and len(r.score_log) == len(r.length_log) == len(r.epsilons) == 1
    # 5 calls banked (1, 2 | 3 episodes | 3 * tick lock-steps) each, at ticks 0 .. 4
    assert list(r.score_log[0]) == [5, 10, 15] and list(r.length_log[0]) == [3 * (0 + 1 + 2 + 3 + 4)]
    assert not r._auto_sums.held.any()                           # zeroed for the next period
    r.run(8)                                                     # ticks 5 .. 12: periods end at 8 and 12
    steps = [i for i, l in enumerate(e.log) if l == "step"]
    assert len(steps) == 13
    calls = [i for i, l in enumerate(e.log) if l.startswith("restart_finished")]
    bots = [i for i, l in enumerate(e.log) if l == "bots"]
    assert len(calls) == len(bots) == 13 and all(c < b for c, b in zip(calls, bots))
    assert all(b < c for b, c in zip(bots, calls[1:]))           # exactly one call per lock-step, at its head
    assert not [l for l in e.log if l.startswith("restart@")]    # restart_random is never called after the spawn
    syncs = [i for i, l in enumerate(e.log) if l == "sync"]
    assert [sum(1 for s in steps if s < i) for i in syncs] == [4, 8, 12]      # the drains: tick % episode_ticks == 0
    assert r.episode == 3 and len(r.score_log) == len(r.length_log) == 3
    assert list(r.length_log[1]) == [3 * (5 + 6 + 7 + 8)] and list(r.score_log[2]) == [4, 8, 12]
    assert r._seen_done.uploads == seen_uploads                  # the latches are never zeroed from the host
    assert r.rung_log == []


def test_auto_reset_with_action_repeat_calls_once_per_decision(fake_buffers):
    e, t, r = _rollout(episode_ticks=8, action_repeat=4, auto_reset=True)
    del e.log[:]
    r.run(5)                                                     # 20 lock-steps: periods end at 8 and 16
    calls = [i for i, l in enumerate(e.log) if l.startswith("restart_finished")]
    spans = [i for i, l in enumerate(e.log) if l.startswith("step_repeat")]
    forwards = [i for i, l in enumerate(e.log) if l == "forward"]
    assert len(calls) == len(spans) == 5 and all(c < f < s for c, f, s in zip(calls, forwards, spans))
    assert e.log[calls[0]].split(":")[3] == "8"                  # max_ticks = episode_ticks, in lock-steps
    assert r.episode == 2 and len(r.length_log) == 2 and not [l for l in e.log if l.startswith("restart@")]


def test_auto_reset_with_the_ladder_groups(fake_buffers):
    e, t = _Engine(N=4), FakeTrainer()
    e.policy_epsilon_ladder = lambda expo: None
    e.restart_finished = lambda seed, ship_mask_ptr=None, **kw: e.log.append(
        "rf:%r:%d:%s" % (kw["group_buf"].ptr, kw["n_groups"], kw["sums_buf"].held.shape))
    r = TrainingRollout(e, t, ["idle", "idle"], seed=3, policy_ships=(0,), episode_ticks=2, epsilon_ladder=1.0,
                        score_bands=2, eval_arenas=1, auto_reset=True)
    G = r.n_groups
    assert G == 3
    r.run(3)
    assert [l for l in e.log if l.startswith("rf")][0] == "rf:%r:%d:%s" % (r._groups.ptr, G, (G, 4))
    assert len(r.rung_log) == 1 and r.rung_log[0].shape == (G, 3) and r.length_log[0].shape == (G,)


@pytest.mark.parametrize("value", [1, 0, None, "yes", 1.0, np.int32(1)])
def test_auto_reset_must_be_a_bool(fake_buffers, value):
    e, t = _Engine(), FakeTrainer()
    with pytest.raises(ValueError) as err:
        TrainingRollout(e, t, ["idle", "idle"], seed=3, auto_reset=value)
    assert "auto_reset" in str(err.value)
    assert e.log == []                                           # before the first device call


# --------------------------------------------------------------------------------------------------- 3. fingerprint
def test_fingerprint_carries_auto_reset_only_when_on(fake_buffers):
    _, _, off = _rollout(episode_ticks=40)
    _, _, on = _rollout(episode_ticks=40, auto_reset=True)
    fp0, fp1 = checkpoint.rollout_fingerprint(off), checkpoint.rollout_fingerprint(on)
    assert "auto_reset" not in fp0 and fp1["auto_reset"] is True
    assert {k: v for k, v in fp1.items() if k != "auto_reset"} == fp0
    for made_by, other, fp in ((on, off, fp1), (off, on, fp0)):  # a checkpoint of one mode is refused by the other
        manifest = {"dims": checkpoint.dims(made_by.e), "trainer_fingerprint": {}, "rollout_fingerprint": fp}
        checkpoint.check(made_by, manifest)
        with pytest.raises(ValueError) as err:
            checkpoint.check(other, manifest)
        assert "rollout.auto_reset " in str(err.value)
