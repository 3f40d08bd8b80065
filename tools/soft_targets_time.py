"""What the soft and Munchausen targets cost (profiles/r21_soft_targets.txt).

head     `--obs` (256) stored observations built on the host (six ship discs of radius 8 and six laser discs of radius 3
         each; beyond 256 the first 256 repeat), the weights pinned.  ofx_policy_profile brackets the streaming head kernel of every forward with an event pair, so the
         figures are the kernel's own time: `--calls` (12) calls each, the first two dropped, of
           default       ofx_policy_forward_obs                        -> k_head_stream<false, 0>
           default_probe the same with a probe                         -> k_head_stream<true, 0>
           soft          ofx_policy_forward_obs_soft at tau_ptr 0.3    -> k_head_stream_soft<false>
           soft_probe    the same with a probe                         -> k_head_stream_soft<true>
           soft_T0       ofx_policy_forward_obs_soft at tau_ptr 0      -> k_head_stream<false, 0>
replay   DeviceTrainer.replay per call at `--arenas` (4096) arenas x 8 ships, one policy ship, memory 64, frames 96,
         fit_batch 256: 40 training lock-steps fill the memories, 5 warm-up replays, then `--repeats` (5) blocks of 20
         replays, ms per replay each.  `--soft` turns soft_targets=(0.5, 0.3) on, `--munchausen` adds munchausen=(0.9, -1)
         (its third forward); without them the file uses only what the trainer had before the options, so it also times a
         copy of the parent commit (`--tree NAME` labels the line).
Usage: python tools/soft_targets_time.py [head] [replay] [--obs 256] [--arenas 4096] [--calls 12] [--repeats 5] [--soft]
                                         [--munchausen] [--tree NAME]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, SEED, SIDE = 8, 0x0F160B21, 400


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ARENAS, N_OBS = _arg("--arenas", 4096), _arg("--obs", 256)


def _observations(n):
    """(bits uint32 [n][2][5000], vec8 float32 [n][8], probe int32 [n][2])"""
    rs = np.random.RandomState(21)
    yy, xx = np.ogrid[:SIDE, :SIDE]
    u = min(n, 256)
    maps = np.zeros((u, 2, SIDE, SIDE), bool)
    for k in range(u):
        for plane, r in ((0, 8), (1, 3)):
            for cy, cx in rs.randint(0, SIDE, (6, 2)):
                maps[k, plane] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    bits = np.packbits(maps.reshape(u, 2, -1), axis=-1, bitorder="little").view(np.uint32)
    bits = np.tile(bits, ((n + u - 1) // u, 1, 1))[:n]
    vec8 = np.tile(np.array([0, 1, 100, 200, SIDE, SIDE, 300, 50], np.float32), (n, 1))
    return np.ascontiguousarray(bits), vec8, rs.randint(0, SIDE, (n, 2)).astype(np.int32)


def head():
    calls = _arg("--calls", 12)
    b = ArenaBatch(8, M)
    w = synthetic()
    dw = DeviceBuffer(w.nbytes).upload(w)
    b.policy_pin_weights(dw.ptr)
    bits, vec8, probe = _observations(N_OBS)
    d_bits, d_vec, d_probe = (DeviceBuffer(a.nbytes).upload(a) for a in (bits, vec8, probe))
    act, ia, ip = DeviceBuffer(8 * N_OBS), DeviceBuffer(4 * N_OBS), DeviceBuffer(8 * N_OBS)
    pm, pp, ps, pz = (DeviceBuffer(4 * N_OBS) for _ in range(4))
    L, h = nat.lib(), b.handle
    common = (h, dw.ptr, N_OBS, d_bits.ptr, d_vec.ptr)
    outs = (act.ptr, ia.ptr, ip.ptr, pm.ptr)

    def soft(tau, with_probe):
        pr = (d_probe.ptr, pp.ptr) if with_probe else (None, None)
        return lambda: nat.check(L.ofx_policy_forward_obs_soft(*common, tau, *outs, *pr, ps.ptr, pz.ptr, None))
    forms = (("default", lambda: nat.check(L.ofx_policy_forward_obs(*common, *outs, None, None))),
             ("default_probe", lambda: nat.check(L.ofx_policy_forward_obs(*common, *outs, d_probe.ptr, pp.ptr))),
             ("soft", soft(0.3, False)), ("soft_probe", soft(0.3, True)), ("soft_T0", soft(0.0, False)))
    out = {"what": "head", "observations": N_OBS, "calls": calls}
    for name, fn in forms:
        b.sync()
        b.policy_profile(0)
        for _ in range(calls):
            fn()
        b.sync()
        b.policy_profile(-1)
        ms = [b.event_elapsed(2 * k, 2 * k + 1) for k in range(2, calls)]
        out[name] = {"head_ms": [round(x, 4) for x in ms], "mean_ms": round(float(np.mean(ms)), 4)}
    out["soft_over_default"] = round(out["soft"]["mean_ms"] / out["default"]["mean_ms"], 3)
    out["soft_probe_over_default_probe"] = round(out["soft_probe"]["mean_ms"] / out["default_probe"]["mean_ms"], 3)
    b.close()
    return out


def replay():
    repeats = _arg("--repeats", 5)
    opt = {}
    if "--soft" in sys.argv or "--munchausen" in sys.argv:
        opt["soft_targets"] = (0.5, 0.3)
    if "--munchausen" in sys.argv:
        opt["munchausen"] = (0.9, -1.0)
    b = ArenaBatch(ARENAS, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=64, frames=96, fit_batch=256, **opt)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=b.cfg.episode_ticks)
    roll.run(40)
    for _ in range(5):
        tr.replay()
    b.sync()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(20):
            tr.replay()
        b.sync()
        ms.append((time.perf_counter() - t0) / 20 * 1e3)
    out = {"what": "replay", "tree": _arg("--tree", "this commit"), "options": {k: list(v) for k, v in opt.items()},
           "arenas": ARENAS, "fit_batch": 256, "ms_per_replay": [round(x, 4) for x in ms], "min_ms": round(min(ms), 4),
           "mean_ms": round(float(np.mean(ms)), 4), "loss": [float(x) for x in tr.losses[-1]]}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("head", "replay")] or ["head", "replay"]
    for name, fn in (("head", head), ("replay", replay)):
        if name in what:
            print(json.dumps(fn()), flush=True)
