"""n-step returns timing: ofx_replay_gather_valid against ofx_replay_gather_nstep at n = 1, 3 and 8 on 256-row and
4096-row windows at 4096 arenas x 400 rows x batch 8 (hipEvents on the handle's stream, after a warm-up), and one 256-row
DeviceTrainer.replay at n_step = 1 and 3 on the same memory (wall time of the call, which ends in the fit's
synchronisation; the two alternate).  Usage: python tools/nstep_time.py [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic
from ofighters_amd.lib.epsilon import Epsilon_decay
from ofighters_amd.trainer import DeviceTrainer
from tools.per_time import BATCH, CAP, M, N, SEED, fill, timed   # the same fill and event timing

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50


def main():
    out = []
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.1)
    tr = DeviceTrainer(b, synthetic(), epsilon=eps, batch_size=BATCH, memory_size=CAP, fit_batch=256, seed=SEED)
    b.spawn_random(SEED)
    fill(b)
    cnt, _ = b.replay_count()
    out.append("arenas %d, rows per arena %d..%d, batch %d, %d reps after 5 warm-up calls" % (N, cnt.min(), cnt.max(), BATCH, REPS))
    slot, n_s = b.replay_sample(SEED, 0, BATCH)
    words = b.W * b.H // 32
    for n in (256, 4096):
        rows = DeviceBuffer(n * b.TRANSITION_DTYPE.itemsize)
        bp, bn = DeviceBuffer(4 * n * 2 * words), DeviceBuffer(4 * n * 2 * words)
        ret, disc = DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        assert b.replay_gather_valid_into(slot, n_s, BATCH, 0, n, rows, bp, bn) == n
        t_v = timed(b, lambda: b.replay_gather_valid_into(slot, n_s, BATCH, 0, n, rows, bp, bn), REPS)
        out.append("ofx_replay_gather_valid        %4d rows  %.4f ms" % (n, t_v))
        for k in (1, 3, 8):
            t_k = timed(b, lambda: b.replay_gather_nstep_into(slot, n_s, BATCH, 0, n, k, 0.9, rows, bp, bn, ret, disc), REPS)
            out.append("ofx_replay_gather_nstep n = %d  %4d rows  %.4f ms  (%.3f x gather_valid)" % (k, n, t_k, t_k / t_v))
        b.sync()
        dc = disc.download(np.float32, (n,))
        g = float(np.float32(0.9))
        full = np.float32(g * g * g * g * g * g * g * g)    # gamma^8 as the contract forms it
        out.append("    (n = 8: %d of %d chains of full length, %d end at a death)" % ((dc == full).sum(), n, (dc == 0).sum()))
        for x in (rows, bp, bn, ret, disc):
            x.free()
    ticks = {1: [], 3: []}
    for k in (1, 3, 1, 3):                    # warm-up: both forms, scratch buffers grown
        tr.n_step = k
        tr.replay()
    b.sync()
    for _ in range(max(5, REPS // 5)):
        for k in (1, 3):
            tr.n_step = k
            t0 = time.perf_counter()
            tr.replay()
            ticks[k].append((time.perf_counter() - t0) * 1e3)
    b.close()
    t1, t3 = float(np.median(ticks[1])), float(np.median(ticks[3]))
    out.append("DeviceTrainer.replay, 256 rows, n_step = 1  %.3f ms (median of %d)" % (t1, len(ticks[1])))
    out.append("DeviceTrainer.replay, 256 rows, n_step = 3  %.3f ms (median of %d)" % (t3, len(ticks[3])))
    out.append("ratio n_step 3 / 1                          %.3f" % (t3 / t1))
    print("\n".join(out))


if __name__ == "__main__":
    main()
