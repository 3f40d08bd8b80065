"""TrainingRollout.checkpoint / restore and DeviceTrainer's state without a device: the stand-ins of
tests/rollout_standin.py extended by what a checkpoint needs, and a DeviceTrainer on host buffers.  A helper module (not
collected); the key lists are the fingerprints' declared content."""
import numpy as np

from ofighters_amd.rollout import TrainingRollout
from tests.rollout_standin import FakeTrainer, MortalEngine, fake_device_buffers

TRAINER_KEYS = ("n_floats", "learning_rate", "gamma", "batch_size", "fit_batch", "seed", "reference_quirks", "prioritized",
                "per_alpha", "per_beta", "per_beta_steps", "per_eps", "n_step", "target_sync", "target_tau", "double_dqn",
                "huber_delta", "clip_norm", "memory_capacity", "memory_frames")
ROLLOUT_KEYS = ("policy_ships", "behaviours", "seed", "episode_ticks", "collecting_steps", "replay_every",
                "replay_on_death", "is_learning")


class CheckpointTrainer(FakeTrainer):
    def __init__(self, uploads, **fp):
        super().__init__()
        self.uploads = uploads
        self.fp = dict({k: 1 for k in TRAINER_KEYS}, learning_rate=1e-3, target_tau=None, reference_quirks=False)
        self.fp.update(fp)
        self.w = np.arange(5, dtype=np.float32)
    def replay(self):
        self.w = self.w + 1
        return super().replay()
    def fingerprint(self): return dict(self.fp)
    def state_dict(self):
        return {"fingerprint": self.fingerprint(), "weights": self.w.copy(), "adam_m": self.w * 2, "adam_v": self.w * 3,
                "target": None, "fit_steps": len(self.replays), "draws": len(self.replays),
                "losses": np.array([(1.0, 2.0)] * len(self.replays)).reshape(-1, 2), "grad_norms": np.zeros(0),
                "epsilon": {"class": "_Eps", "attrs": {"v": self.epsilon.v, "n": self.epsilon.n}}}
    def load_state_dict(self, d):
        self.uploads.append("trainer")
        self.w = d["weights"].copy()
        self.replays = list(range(d["fit_steps"]))
        self.epsilon.v, self.epsilon.n = d["epsilon"]["attrs"]["v"], d["epsilon"]["attrs"]["n"]


class CheckpointEngine(MortalEngine):
    """The mortal stand-in with a replay memory of four bytes per arena and what a checkpoint needs."""
    def __init__(self, uploads, N=3, M=2, arena_base=0):
        super().__init__(N, M, arena_base)
        self.uploads, self.fail_export = uploads, False
        self.memory = np.zeros((N, 4), np.uint8)
    def replay_capture(self, tick, ship_mask_ptr=None):
        super().replay_capture(tick)
        self.memory[:, tick % 4] = tick % 251
    def state_dict(self): return {"ship_alive": self.alive.copy(), "time": np.full(self.N, self.t, np.int32),
                                  "episode": self.episode, "tick": self.t}
    def load_state_dict(self, d):
        self.uploads.append("arena")
        self.alive, self.t, self.episode = d["ship_alive"].copy(), int(d["time"][0]), d["episode"]
    def replay_export_bytes(self, a, n): return 4 * n
    def replay_export(self, a, n):
        if self.fail_export and a > 0:
            raise RuntimeError("export interrupted")
        return self.memory[a:a + n].reshape(-1).copy()
    def replay_import(self, a, n, blob):
        self.uploads.append("replay:%d:%d" % (a, n))
        self.memory[a:a + n] = np.asarray(blob).reshape(n, 4)


def standins(monkeypatch, tmp_path, engine_kw=None, trainer_fp=None, engine=CheckpointEngine, **roll_kw):
    """-> (rollout, engine, trainer, uploads): a TrainingRollout on the stand-ins; uploads logs what a restore writes"""
    uploads = []
    fake_device_buffers(monkeypatch, uploads)
    e, t = engine(uploads, **(engine_kw or {})), CheckpointTrainer(uploads, **(trainer_fp or {}))
    kw = dict(seed=3, policy_ships=(0,), episode_ticks=40, snapshot_every=2, snapshot_folder=str(tmp_path / "snap"),
              collecting_steps=20, replay_every=50)
    kw.update(roll_kw)
    r = TrainingRollout(e, t, kw.pop("behaviours", ["idle", "idle"]), **kw)
    t.clock = lambda: r.total_steps
    del uploads[:]
    return r, e, t, uploads


# ------------------------------------------------------------------------- DeviceTrainer on host buffers
class HostBuffer:
    """DeviceBuffer stand-in holding its bytes on the host."""
    log = []
    def __init__(self, nbytes): self.nbytes, self.data, self.ptr = int(nbytes), np.zeros(int(nbytes), np.uint8), 1
    def upload(self, arr):
        HostBuffer.log.append(self)
        b = np.ascontiguousarray(arr).reshape(-1).view(np.uint8)
        self.data[:b.size] = b
        return self
    def download(self, dtype, shape, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.data[offset:offset + n].view(dtype).reshape(shape).copy()
    def free(self): pass


class FakeBatch:
    N, M = 2, 2
    def sync(self): pass
    def replay_create(self, capacity, frames=0):
        self.replay_capacity, self.replay_frames = capacity, frames or capacity + capacity // 4 + 2
    def replay_prioritize(self, alpha, eps): self.replay_prioritized = True


BASE = dict(learning_rate=1e-3, batch_size=4, memory_size=16, frames=0, seed=5, fit_batch=16, prioritized=True, n_step=3,
            target_sync=2, double_dqn=True, huber_delta=1.0, clip_norm=10.0)


def host_trainer(monkeypatch, n_floats=6, **kw):
    import ofighters_amd.trainer as tr
    from ofighters_amd.lib.epsilon import Epsilon_decay
    monkeypatch.setattr(tr, "DeviceBuffer", HostBuffer)
    return tr.DeviceTrainer(FakeBatch(), np.arange(n_floats, dtype=np.float32), epsilon=Epsilon_decay(), **dict(BASE, **kw))
