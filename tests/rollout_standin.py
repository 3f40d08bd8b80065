"""The recording stand-ins TrainingRollout's CPU tests run against: an engine that logs the call order of a lock-step, a
trainer that logs its replays, and a host-side DeviceBuffer.  A helper module (not collected).  What only one option's
test needs - step_repeat, restart_finished, the ladder calls, whether spawn / restart / sync are logged - is a subclass
in that test's own file."""
import numpy as np


class Buf:
    ptr = 1


class Eps:
    def __init__(self): self.v, self.n = 0.5, 0
    def get(self): return self.v
    def next(self): self.n += 1


class FakeTrainer:
    """`clock` is set by the test once the rollout exists: replays records what it reads at every replay."""
    def __init__(self):
        self.weights, self.epsilon, self.replays, self.saved = Buf(), Eps(), [], []
    def decay_epsilon(self): self.epsilon.next()
    def replay(self):
        self.replays.append(self.clock())
        return (1.0, 2.0)
    def save(self, id=None, overwrite=False, folder=None):
        self.saved.append(id)
        return "%s/%s" % (folder, id)
    def fingerprint(self): return {}


class FakeEngine:
    """Records the call order of one lock-step; nobody dies."""
    W = H = 400
    def __init__(self, N=3, M=2, arena_base=0):
        self.N, self.M, self.arena_base = N, M, arena_base
        self.episode, self.log, self.tick = 0, [], 0
    def sync(self): pass
    def spawn_random(self, seed): pass
    def restart_random(self, seed): self.episode += 1
    def episode_scores(self): return np.arange(self.M + 1, dtype=np.int64)
    def policy_pin_weights(self, p): self.log.append("pin")
    def agents_first_done(self, mask_ptr, seen): return 0
    def bot_actions(self, beh, seed, tick=None): self.log.append("bots")
    def policy_forward(self, w, m): self.log.append("forward")
    def policy_explore(self, eps, seed, tick=None, collecting=False, ship_mask_ptr=None):
        self.log.append("explore:%d:%d" % (tick, collecting))
    def replay_capture(self, tick, ship_mask_ptr=None): self.log.append("capture:%d" % tick)
    def policy_actions(self, ship_mask_ptr=None): self.log.append("actions")
    def step(self):
        self.log.append("step")
        self.tick += 1
    def rasterise(self): self.log.append("raster")


class MortalEngine(FakeEngine):
    """Ship 0 of arena 1 dies at tick 7 of every episode (`t`: the episode's own clock)."""
    def __init__(self, N=3, M=2, arena_base=0):
        super().__init__(N, M, arena_base)
        self.t = 0
        self.alive = np.ones((N, M), np.uint8)
        self.seen = np.zeros((N, M), bool)
        self.mask = np.zeros((N, M), bool); self.mask[:, 0] = True
    def restart_random(self, seed):
        self.episode += 1; self.alive[:] = 1; self.t = 0
    def get(self, field): return self.alive.copy()
    def agents_first_done(self, mask_ptr, seen):          # the device-side `done` latches (ofx_agents_first_done)
        if getattr(seen, "cleared", False): self.seen, seen.cleared = np.zeros((self.N, self.M), bool), False
        first = (self.alive == 0) & self.mask & ~self.seen
        self.seen |= first
        return int(first.sum())
    def step(self):
        super().step(); self.t += 1
        if self.t == 7: self.alive[1, 0] = 0


def fake_device_buffers(monkeypatch, log=None):
    """Put a host-side DeviceBuffer into ofighters_amd.engine -> the list of the buffers made since.  A buffer holds what
    was uploaded last (`held`, also read as `data`), counts its uploads, answers download from it, and carries `cleared`:
    TrainingRollout zeroes the latches at episode ends.  log: a list that gets "buffer" at every upload."""
    import ofighters_amd.engine as eng
    made = []

    class DB:
        data = property(lambda self: self.held)
        def __init__(self, n):
            made.append(self)
            self.ptr, self.uploads = 100 + len(made), 0
        def upload(self, a):
            self.held = np.array(a)
            self.cleared = not self.held.any()
            self.uploads += 1
            if log is not None:
                log.append("buffer")
            return self
        def download(self, dtype, shape):
            return np.array(self.held, dtype).reshape(shape)
    monkeypatch.setattr(eng, "DeviceBuffer", DB)
    return made
