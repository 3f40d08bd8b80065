"""Packed frame store against the dense frame ring at the training tick's size (profiles/r09_packed_replay.txt): 4096
arenas x 8 ships, one policy ship, memory_size 400, the memory filled by the training tick itself (TrainingRollout,
["random"] * 8, episode_ticks 200, batch_size 8, fit_batch 256).  Per form, after `--steps` training lock-steps:
the frame store's numbers (ArenaBatch.replay_store_stats), then `--reps` times each of
  tick     wall time per lock-step of 200 further training lock-steps (ends in a synchronise)
  capture  ofx_replay_capture per call, HIP events on the handle's stream around 100 single calls (raster + bookkeeping +
           the frame kernel), a lock-step between two calls
  replay   wall time of one DeviceTrainer.replay at fit_batch 256, median of 20 (the call ends in the fit's synchronise)
Usage: python tools/packed_replay_time.py [--steps 2500] [--reps 3] [--dense-only] [--package DIR] [--big]
--dense-only times the dense ring alone and uses nothing the packed store added, so with --package DIR (import
ofighters_amd from DIR instead of this tree) it runs on a checkout from before it: two builds on one card in one session.
--big instead builds DeviceTrainer(packed_memory=True) at 32 768 arenas (BASELINE configs[4]), runs 100 training
lock-steps and prints the store's numbers and the free HBM."""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


PKG = os.path.abspath(_arg("--package", ROOT))
sys.path.insert(0, PKG)
import numpy as np

from ofighters_amd import ArenaBatch
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.rollout import TrainingRollout
from ofighters_amd.trainer import DeviceTrainer

M, CAP, SEED = 8, 400, 0x0F160051
STEPS, REPS = _arg("--steps", 2500), _arg("--reps", 3)


def build(n_arenas, packed):
    b = ArenaBatch(n_arenas, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    kw = dict(packed_memory=True) if packed else {}          # nothing new is named on the dense path (--package)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=8, memory_size=CAP, fit_batch=256, seed=SEED, **kw)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0,), episode_ticks=200)
    return b, tr, roll


def free_hbm():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value), int(total.value)


def run(b, roll, n):
    t0 = time.perf_counter()
    roll.run(n)
    b.sync()
    return time.perf_counter() - t0


def measure(form):
    b, tr, roll = build(4096, form == "packed")
    out = {"form": form, "fill_steps": STEPS, "fill_s": run(b, roll, STEPS), "fits": tr.fit_steps}
    if hasattr(b, "replay_store_stats"):
        out["stats"] = b.replay_store_stats()
    out["free_hbm"] = free_hbm()[0]
    out["tick_ms"], out["capture_ms"], out["replay_ms"] = [], [], []
    for _ in range(REPS):
        out["tick_ms"].append(run(b, roll, 200) / 200 * 1e3)
        ms = []
        for _ in range(100):                                   # the rollout's own capture, alone between two events
            b.bot_actions(["random"] * M, SEED, tick=roll.tick)
            b.timer_start()
            b.replay_capture(roll.capture_tick, ship_mask_ptr=roll._mask.ptr)
            ms.append(b.timer_stop())
            roll.capture_tick += 1
            b.step()
        out["capture_ms"].append(float(np.mean(ms[10:])))
        ts = []
        for _ in range(23):
            t0 = time.perf_counter()
            tr.replay()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["replay_ms"].append(float(np.median(ts[3:])))
    if "stats" in out:
        out["stats_end"] = b.replay_store_stats()
    b.close()
    return out


def big():
    free0, total = free_hbm()
    b, tr, roll = build(32768, True)
    out = {"arenas": 32768, "hbm_total": total, "free_before": free0, "free_after_create": free_hbm()[0],
           "stats_create": b.replay_store_stats(), "steps": 100, "s": run(b, roll, 100), "fits": tr.fit_steps,
           "losses_finite": bool(np.isfinite(np.array(tr.losses)).all()), "stats": b.replay_store_stats(),
           "free_after_run": free_hbm()[0], "rows": int(b.replay_count()[0].sum())}
    b.close()
    return out


if __name__ == "__main__":
    print(json.dumps({"package": os.path.relpath(PKG, ROOT), "argv": sys.argv[1:]}))
    if "--big" in sys.argv:
        print(json.dumps(big()))
    else:
        for form in ("dense",) if "--dense-only" in sys.argv else ("dense", "packed"):
            print(json.dumps(measure(form)), flush=True)
