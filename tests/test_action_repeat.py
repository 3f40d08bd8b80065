"""Action repeat on the CPU: the model the GPU tests compare against (tests/repeat_oracle.py) exercises what it must, and
TrainingRollout(action_repeat=K) makes the calls, counts the decisions and refuses the arguments the way its docstring
says - against a recording stand-in for the engine, like tests/test_learning_loop.py."""
import numpy as np
import pytest

from ofighters_amd import checkpoint
from ofighters_amd.rollout import TrainingRollout
from tests import repeat_oracle as ro
from tests.rollout_standin import FakeEngine, FakeTrainer, fake_device_buffers


# ------------------------------------------------------------------------------------------------- 1. the model
def test_span_oracle_is_the_sequential_composition():
    """span_oracle(K) == K x span_oracle(1) on a twin, and a held ship really plays its action, not its behaviour."""
    from oracle import pyoracle
    beh = np.array([ro.BOT[b] for b in ro.BEHAVIOURS], np.int32)
    a, b = ro.spawn(ro.SEED, 1)[0], ro.spawn(ro.SEED, 1)[0]
    held = {0: (1, 0, 1, 399, 399), 3: (1, 1, 0, 0, 0)}
    start = a.ships()["xy"].copy()
    ra = ro.span_oracle(a, beh, ro.SEED, 0, 0, 3, held)
    rb = np.concatenate([ro.span_oracle(b, beh, ro.SEED, 0, j, 1, held) for j in range(3)])
    assert np.array_equal(ra, rb)
    sa, sb = a.ships(), b.ships()
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert tuple(sa["pt"][0]) == (399, 399) and tuple(sa["pt"][3]) == (0, 0)
    assert not np.array_equal(sa["xy"][0], start[0])            # ship 0's behaviour is "shoot": it never thrusts itself
    assert np.array_equal(sa["xy"][3], start[3])                # the held ship 3 only shoots


def test_scenario_conditions():
    """The four conditions without which the GPU comparison would be vacuous, over the held ships of the scenario."""
    sc = ro.scenario()
    held = list(ro.HELD)
    rew = sc["rewards"][:, :, :, held]                          # [spans][K][N][held]
    before = sc["alive_before"][:, :, :, held]
    alive0 = sc["alive0"][:, :, held]                           # [spans][N][held]
    # a ship alive at the decision that is dead when the span's LAST lock-step begins died before that lock-step
    early_deaths = int(((alive0 == 1) & (before[:, -1] == 0)).sum())
    multi = int(((rew != 0).sum(axis=1) >= 2).sum())
    sum_differs = int((rew.sum(axis=1) != rew[:, -1]).sum())
    posthumous = int(((before == 0) & (rew != 0)).sum())
    print("early deaths %d, spans with >= 2 rewarded lock-steps %d, sum != last %d, rewards to a dead ship %d"
          % (early_deaths, multi, sum_differs, posthumous))
    assert early_deaths >= 1
    assert multi >= 1
    assert sum_differs >= 1
    assert posthumous >= 1
    acts = sc["actions"][:, :, held]
    assert np.array_equal(acts[..., 0], alive0) and (acts[..., 1] + acts[..., 2] == 1).all()


# ------------------------------------------------------------------------------------------- 2. the call sequence
class _Engine(FakeEngine):
    """The stand-in with the span calls; spawn and restart are logged."""
    def spawn_random(self, seed): self.log.append("spawn")
    def restart_random(self, seed):
        self.episode += 1
        self.log.append("restart@%d" % self.tick)
    def replay_reward_source(self, ptr): self.log.append("reward_source:%r" % ptr)
    def step_repeat(self, behaviours, seed, tick0, n_ticks, hold_mask_ptr=None, actions_ptr=None, span_reward_ptr=None,
                    observe=None):
        self.log.append("step_repeat:%d:%d:%r:%r:%r:%r" % (tick0, n_ticks, hold_mask_ptr, actions_ptr, span_reward_ptr,
                                                            observe))
        self.tick += n_ticks


@pytest.fixture
def fake_buffers(monkeypatch):
    return fake_device_buffers(monkeypatch)


def _rollout(**kw):
    e, t = _Engine(), FakeTrainer()
    r = TrainingRollout(e, t, ["idle", "idle"], seed=3, policy_ships=(0,), collecting_steps=3, replay_every=5, **kw)
    t.clock = lambda: r.total_steps
    return e, t, r


def test_action_repeat_1_is_todays_call_sequence(fake_buffers):
    e, t, r = _rollout(episode_ticks=40, action_repeat=1)
    r.run(2)
    assert e.log == ["spawn", "pin",
                     "bots", "forward", "explore:0:1", "capture:0", "actions", "step", "raster",
                     "bots", "forward", "explore:1:1", "capture:1", "actions", "step", "raster"]
    assert r.tick == 2 and r.action_repeat == 1 and not hasattr(r, "_span")
    e2, t2, r2 = _rollout(episode_ticks=40)                     # the default is off
    r2.run(2)
    assert e2.log == e.log


def test_action_repeat_4_one_span_per_decision(fake_buffers):
    from ofighters_amd import _native as nat
    e, t, r = _rollout(episode_ticks=8, action_repeat=4)
    mask, span = r._mask.ptr, r._span.ptr
    assert span != mask and r._span.held.dtype == np.int32 and r._span.held.shape == (3, 2) and not r._span.held.any()
    assert e.log == ["spawn", "pin", "reward_source:%r" % span]
    del e.log[:]
    r.run(1)
    assert e.log == ["forward", "explore:0:1", "capture:0", "actions",
                     "step_repeat:0:4:%r:None:%r:%r" % (mask, span, nat.MAP_U8)]
    assert r.tick == 4 and e.tick == 4 and r.total_steps == 1 and r.capture_tick == 1
    r.run(6)                                                    # 7 decisions = 28 lock-steps: episodes end at 8, 16, 24
    assert r.tick == 28 and e.tick == 28 and r.total_steps == 7 and r.capture_tick == 7
    assert not [l for l in e.log if l in ("bots", "step", "raster")]
    assert [l.split(":")[1] for l in e.log if l.startswith("step_repeat")] == ["0", "4", "8", "12", "16", "20", "24"]
    assert [l for l in e.log if l.startswith("restart")] == ["restart@8", "restart@16", "restart@24"]
    assert len([l for l in e.log if l.startswith("reward_source")]) == 0      # registered once, in the constructor
    assert r.episode == 3
    # the schedules count decisions: collecting while total_steps < 3, a replay at every 5th decision, one decay per
    # decision after the collecting phase
    assert [l for l in e.log if l.startswith("explore")][:4] == ["explore:0:1", "explore:1:1", "explore:2:0", "explore:3:0"]
    assert t.replays == [5] and t.epsilon.n == 7 - 2
    # the probe brackets the span like the headless loop does: (stage, begin, n lock-steps)
    seen = []
    r.probe = lambda *a: seen.append(a)
    r.run(1)
    assert seen == [("step", True, 4), ("step", False, 4)]
    # observe=False: no maps
    e3, t3, r3 = _rollout(episode_ticks=8, action_repeat=2, observe=False)
    r3.run(1)
    assert e3.log[-1].endswith(":None") and e3.log[-1].startswith("step_repeat:0:2:")


@pytest.mark.parametrize("kw", [dict(action_repeat=True), dict(action_repeat=0), dict(action_repeat=2.0),
                                dict(action_repeat="2"), dict(action_repeat=-3),
                                dict(action_repeat=3, episode_ticks=40),
                                dict(action_repeat=4, episode_ticks=40, start_tick=6)])
def test_action_repeat_value_errors(fake_buffers, kw):
    e, t = _Engine(), FakeTrainer()
    with pytest.raises(ValueError) as err:
        TrainingRollout(e, t, ["idle", "idle"], seed=3, **kw)
    assert "action_repeat" in str(err.value)
    assert e.log == []                                          # before the first device call


# --------------------------------------------------------------------------------------------------- 3. fingerprint
def test_fingerprint_carries_action_repeat_only_when_on(fake_buffers):
    _, _, r1 = _rollout(episode_ticks=40, action_repeat=1)
    _, _, r4 = _rollout(episode_ticks=40, action_repeat=4)
    _, _, r2 = _rollout(episode_ticks=40, action_repeat=2)
    fp1, fp4 = checkpoint.rollout_fingerprint(r1), checkpoint.rollout_fingerprint(r4)
    assert "action_repeat" not in fp1 and fp4["action_repeat"] == 4
    assert {k: v for k, v in fp4.items() if k != "action_repeat"} == fp1
    manifest = {"dims": checkpoint.dims(r4.e), "trainer_fingerprint": {}, "rollout_fingerprint": fp4}
    checkpoint.check(r4, manifest)
    for other in (r2, r1):
        with pytest.raises(ValueError) as err:
            checkpoint.check(other, manifest)
        assert "rollout.action_repeat " in str(err.value)
