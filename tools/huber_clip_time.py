"""Huber loss / gradient-norm clip timing: one 256-row DeviceTrainer.replay on a 4096-arena memory (400 rows per arena,
batch 8), without the two options and with huber_delta = 1.0 + clip_norm = 1.0, the two alternating on the same trainer
(wall time of the call, which ends in the fit's synchronisation; median and range).  What the options are expected to
add is one pass over the gradient blob, the one-thread tail and Adam's read of the factor.
Usage: python tools/huber_clip_time.py [reps] [--plain-only] [--package DIR]
--plain-only times the replay without the options alone (it then runs on a checkout that has no ofx_dqn_fit_robust);
--package DIR imports ofighters_amd from DIR instead of this tree, to compare two builds on one card in one session."""
import os
import sys
import time

ARGS = [a for a in sys.argv[1:] if not a.startswith("--")]
PLAIN_ONLY = "--plain-only" in sys.argv
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--package" in sys.argv:
    PKG = os.path.abspath(sys.argv[sys.argv.index("--package") + 1])
    ARGS = [a for a in ARGS if os.path.abspath(a) != PKG]
    sys.path.insert(0, PKG)
    sys.path.insert(1, ROOT)
else:
    PKG = ROOT
    sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.trainer import DeviceTrainer
from tools.per_time import BATCH, CAP, M, N, SEED, fill   # the same fill

REPS = int(ARGS[0]) if ARGS else 50
MODES = ("plain",) if PLAIN_ONLY else ("plain", "huber + clip")


def set_mode(tr, mode):
    if PLAIN_ONLY:
        return
    tr.huber_delta = None if mode == "plain" else 1.0
    tr.clip_norm = None if mode == "plain" else 1.0


def main():
    out = ["package %s%s" % (os.path.relpath(PKG, ROOT), ", plain only" if PLAIN_ONLY else "")]
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=BATCH, memory_size=CAP, fit_batch=256, seed=SEED)
    b.spawn_random(SEED)
    fill(b)
    cnt, _ = b.replay_count()
    out.append("arenas %d, rows per arena %d..%d, batch %d, fit_batch 256, %d replays per form after 3 warm-up replays each" %
               (N, cnt.min(), cnt.max(), BATCH, REPS))
    ticks = {m: [] for m in MODES}
    for m in MODES * 3:                          # warm-up: both forms, scratch buffers and workspace grown
        set_mode(tr, m)
        tr.replay()
    b.sync()
    for _ in range(REPS):
        for m in MODES:
            set_mode(tr, m)
            t0 = time.perf_counter()
            tr.replay()
            ticks[m].append((time.perf_counter() - t0) * 1e3)
    med = {m: float(np.median(ticks[m])) for m in MODES}
    for m in MODES:
        out.append("DeviceTrainer.replay 256 rows  %-13s %8.3f ms  (min %.3f, max %.3f)" % (m, med[m], min(ticks[m]), max(ticks[m])))
    if not PLAIN_ONLY:
        out.append("ratio huber + clip / plain (this build)  %.3f" % (med["huber + clip"] / med["plain"]))
        norms = np.array(tr.grad_norms)
        out.append("gradient norms of the timed steps: median %.4g, clipped on %d of %d" %
                   (np.median(norms), (norms > 1.0).sum(), len(norms)))
    b.close()
    print("\n".join(out))


if __name__ == "__main__":
    main()
