"""Prioritized replay timing: the PER kernels at 4096 arenas x 400 rows x batch 8 (hipEvents on the handle's stream,
after a warm-up; the uniform sampler beside them), and one 256-row DeviceTrainer.replay with PER on and off (wall time
of the call, which ends in the fit's synchronisation).  Usage: python tools/per_time.py [reps] [--package DIR]
--package DIR imports ofighters_amd from DIR instead of this tree (tools/global_replay_time.py's option): two builds on
one card in one session."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = ROOT
if "--package" in sys.argv:
    at = sys.argv.index("--package")
    PKG = os.path.abspath(sys.argv[at + 1])
    del sys.argv[at:at + 2]
sys.path.insert(0, PKG)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.trainer import DeviceTrainer

N, M, CAP, BATCH, SEED = 4096, 8, 400, 8, 0x0F160041
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def fill(b):
    """every ship captures on every lock-step (8 rows per arena and tick while all live); a new episode every 20
    lock-steps, until every memory holds CAP rows"""
    ia, ip = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(400):
        if t and t % 20 == 0:
            b.sync()
            if b.replay_count()[0].min() == CAP:
                break
            b.restart_random(SEED)
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.policy_explore(1.0, SEED, tick=t, collecting=True, iaction_ptr=ia.ptr, ipointer_ptr=ip.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, iaction_ptr=ia.ptr, ipointer_ptr=ip.ptr)
        b.replay_capture(t, None, ia.ptr, ip.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()


def timed(b, fn, reps):
    for _ in range(5):
        fn()
    b.sync()
    b.event_record(0)
    for _ in range(reps):
        fn()
    b.event_record(1)
    return b.event_elapsed(0, 1) / reps


def trainer(prioritized):
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=BATCH, memory_size=CAP, fit_batch=256, seed=SEED,
                       prioritized=prioritized)
    b.spawn_random(SEED)
    fill(b)
    return b, tr


def main():
    out = ["package %s" % os.path.relpath(PKG, ROOT)]
    b, tr = trainer(True)
    cnt, _ = b.replay_count()
    out.append("arenas %d, rows per arena %d..%d, batch %d, %d reps after 5 warm-up calls" % (N, cnt.min(), cnt.max(), BATCH, REPS))
    for _ in range(20):                      # priorities that are not all equal
        tr.replay()
    slot, n_s, isw = DeviceBuffer(4 * N * BATCH), DeviceBuffer(4 * N), DeviceBuffer(4 * N * BATCH)
    b.replay_sample_prioritized(SEED, 0, BATCH, 0.4, slot, n_s, isw)
    n = 256
    rows = DeviceBuffer(n * b.TRANSITION_DTYPE.itemsize)
    words = b.W * b.H // 32
    bp, bn = DeviceBuffer(4 * n * 2 * words), DeviceBuffer(4 * n * 2 * words)
    assert b.replay_gather_valid_into(slot, n_s, BATCH, 0, n, rows, bp, bn) == n
    wts, td = DeviceBuffer(4 * n), DeviceBuffer(8 * n)
    td.upload(np.random.RandomState(0).normal(0, 1, (n, 2)).astype(np.float32))
    t_s = timed(b, lambda: b.replay_sample_prioritized(SEED, 1, BATCH, 0.4, slot, n_s, isw), REPS)
    t_w = timed(b, lambda: b.replay_window_weights_into(isw, n_s, BATCH, 0, n, wts), REPS)
    t_u = timed(b, lambda: b.replay_update_priorities(slot, n_s, BATCH, 0, n, rows.ptr, td.ptr), REPS)
    t_uni = timed(b, lambda: b.replay_sample(SEED, 1, BATCH, slot, n_s), REPS)
    out.append("ofx_replay_sample_prioritized  %.4f ms" % t_s)
    out.append("ofx_replay_window_weights      %.4f ms  (256-row window)" % t_w)
    out.append("ofx_replay_update_priorities   %.4f ms  (256-row window)" % t_u)
    out.append("sampler + window + update      %.4f ms" % (t_s + t_w + t_u))
    out.append("ofx_replay_sample (uniform)    %.4f ms" % t_uni)
    ticks = {}
    for per in (True, False):
        if not per:
            b.close()
            b, tr = trainer(False)
        for _ in range(3):
            tr.replay()
        b.sync()
        ts = []
        for _ in range(max(5, REPS // 5)):
            t0 = time.perf_counter()
            tr.replay()
            ts.append((time.perf_counter() - t0) * 1e3)
        ticks[per] = float(np.median(ts))
    b.close()
    out.append("DeviceTrainer.replay, 256 rows, PER on   %.3f ms (median)" % ticks[True])
    out.append("DeviceTrainer.replay, 256 rows, PER off  %.3f ms (median)" % ticks[False])
    out.append("ratio on / off                            %.3f" % (ticks[True] / ticks[False]))
    print("\n".join(out))


if __name__ == "__main__":
    main()
