"""Target network / Double DQN timing: one DeviceTrainer.replay at fit_batch 256 and 4096 on a 4096-arena memory (400
rows per arena, batch 8) - plain, with target_sync, with double_dqn + target_sync, the three alternating on the same
trainer (wall time of the call, which ends in the fit's synchronisation; median and range) - and beside them a stand-alone
ofx_policy_forward_obs on as many rows (hipEvents on the handle's stream), without and with a probe: what double_dqn is
expected to add is one forward on next_state.  target_sync is 1 here, so every replay pays the copy.
Usage: python tools/double_dqn_time.py [reps] [--plain-only] [--package DIR]
--plain-only times the plain replay and the forward alone (it then runs on a checkout that has no target network);
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

from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.trainer import DeviceTrainer
from tools.per_time import BATCH, CAP, M, N, SEED, fill, timed   # the same fill and event timing

REPS = int(ARGS[0]) if ARGS else 20
MODES = ("plain",) if PLAIN_ONLY else ("plain", "target_sync", "double_dqn + target_sync")


def set_mode(tr, mode, target):
    if PLAIN_ONLY:
        return
    tr.target = None if mode == "plain" else target
    tr.target_sync = 0 if mode == "plain" else 1
    tr.double_dqn = mode.startswith("double")


def main():
    out = ["package %s%s" % (os.path.relpath(PKG, ROOT), ", plain only" if PLAIN_ONLY else "")]
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    w = synthetic()
    tr = DeviceTrainer(b, w, epsilon=eps, batch_size=BATCH, memory_size=CAP, fit_batch=256, seed=SEED)
    target = DeviceBuffer(w.nbytes).upload(w)
    b.spawn_random(SEED)
    fill(b)
    cnt, _ = b.replay_count()
    out.append("arenas %d, rows per arena %d..%d, batch %d, %d replays per form after 2 warm-up replays each" %
               (N, cnt.min(), cnt.max(), BATCH, REPS))
    for n in (256, 4096):
        tr.fit_batch = n
        ticks = {m: [] for m in MODES}
        for m in MODES + MODES:                  # warm-up: every form, scratch buffers and workspace grown
            set_mode(tr, m, target)
            tr.replay()
        b.sync()
        for _ in range(REPS):
            for m in MODES:
                set_mode(tr, m, target)
                t0 = time.perf_counter()
                tr.replay()
                ticks[m].append((time.perf_counter() - t0) * 1e3)
        med = {m: float(np.median(ticks[m])) for m in MODES}
        for m in MODES:
            out.append("DeviceTrainer.replay %4d rows  %-25s %8.3f ms  (min %.3f, max %.3f; + %.3f ms over plain)" %
                       (n, m, med[m], min(ticks[m]), max(ticks[m]), med[m] - med["plain"]))
        # the forward the targets run, on the window the last replay gathered
        rows_h = tr._buf["rows"].download(b.TRANSITION_DTYPE, (n,))
        vec = DeviceBuffer(32 * n).upload(np.ascontiguousarray(rows_h["head_next"], np.float32))
        act, pmax, ia, ip, probe = DeviceBuffer(8 * n), DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n)
        bits, wp, h, L = tr._buf["bits_next"].ptr, tr.weights.ptr, b.handle, nat.lib()
        t_max = timed(b, lambda: nat.check(L.ofx_policy_forward_obs(h, wp, n, bits, vec.ptr, act.ptr, None, None, pmax.ptr,
                                                                      None, None)), REPS)
        nat.check(L.ofx_policy_forward_obs(h, wp, n, bits, vec.ptr, None, ia.ptr, ip.ptr, None, None, None))
        t_probe = timed(b, lambda: nat.check(L.ofx_policy_forward_obs(h, wp, n, bits, vec.ptr, act.ptr, None, None, None,
                                                                        ip.ptr, probe.ptr)), REPS)
        out.append("ofx_policy_forward_obs %4d rows  ptr_max %8.3f ms   with a probe %8.3f ms" % (n, t_max, t_probe))
        b.sync()
        for x in (vec, act, pmax, ia, ip, probe):
            x.free()
    b.close()
    print("\n".join(out))


if __name__ == "__main__":
    main()
