"""TrainingRollout._play on a stand-in that records every call with its arguments: the helper of tests/test_boltzmann.py
and tests/record_play_calls.py (not collected).  The engine subclasses the mortal stand-in of tests/rollout_standin.py, so
the runs hold deaths, replays, a collecting phase and episode ends."""
import numpy as np

from tests.rollout_standin import FakeTrainer, MortalEngine


class PlayEngine(MortalEngine):
    """Logs (name, arguments) of every engine call of a lock-step.  `calls` counts the calls made before the rollout's
    constructor returns or raises: a bad argument must be refused before the first one."""
    def __init__(self, N=3, M=2, arena_base=0):
        super().__init__(N, M, arena_base)
        self.calls = 0

    def _rec(self, name, *args):
        self.calls += 1
        self.log.append([name] + [a.item() if isinstance(a, np.generic) else a for a in args])

    def sync(self): self.calls += 1
    def spawn_random(self, seed): self.calls += 1
    def policy_pin_weights(self, p): self._rec("pin", p)
    def policy_epsilon_ladder(self, expo): self._rec("ladder", [repr(float(x)) for x in expo])
    def episode_scores_grouped(self, groups, n): return np.zeros((n, self.M + 1), np.int64)
    def bot_actions(self, beh, seed, tick=None): self._rec("bots", list(beh), seed, tick)
    def policy_forward(self, w, m): self._rec("forward", w, m)
    def policy_explore(self, eps, seed, tick=None, collecting=False, ship_mask_ptr=None):
        self._rec("explore", eps, seed, tick, bool(collecting), ship_mask_ptr)
    def policy_act(self, w, eps, seed, tick=None, collecting=False, ship_mask_ptr=None):
        self._rec("act", w, eps, seed, tick, bool(collecting), ship_mask_ptr)
    def policy_act_boltzmann(self, w, eps, tau_act, tau_ptr, seed, tick=None, collecting=False, ship_mask_ptr=None):
        self._rec("act_boltzmann", w, eps, tau_act, tau_ptr, seed, tick, bool(collecting), ship_mask_ptr)
    def replay_capture(self, tick, ship_mask_ptr=None): self._rec("capture", tick, ship_mask_ptr)
    def replay_capture_valued(self, tick, ship_mask_ptr=None): self._rec("capture_valued", tick, ship_mask_ptr)
    def policy_actions(self, ship_mask_ptr=None): self._rec("actions", ship_mask_ptr)
    def rasterise(self): self._rec("raster")


class PlayTrainer(FakeTrainer):
    def __init__(self, actor_priorities=False):
        super().__init__()
        self.actor_priorities = actor_priorities
    def decay_epsilon(self):
        super().decay_epsilon()
        self.epsilon.v *= 0.99


# name -> (trainer arguments, TrainingRollout arguments): the option under test is off in all of them
OFF_CASES = {
    "default": ({}, {}),
    "actor_priorities": ({"actor_priorities": True}, {}),
    "eval_arena": ({"actor_priorities": True}, {"eval_arenas": 1}),
}
STEPS = 30


def run_case(rollout_module, fake_buffers, trainer_kw, rollout_kw):
    """-> the engine's log over STEPS lock-steps (JSON-ready) of rollout_module.TrainingRollout on the stand-ins."""
    fake_buffers()
    e, t = PlayEngine(), PlayTrainer(**trainer_kw)
    kw = dict(seed=3, policy_ships=(0,), episode_ticks=10, collecting_steps=5, replay_every=7)
    kw.update(rollout_kw)
    r = rollout_module.TrainingRollout(e, t, ["idle", "idle"], **kw)
    t.clock = lambda: r.total_steps
    r.run(STEPS)
    return {"log": e.log, "replays": t.replays, "capture_tick": r.capture_tick}
