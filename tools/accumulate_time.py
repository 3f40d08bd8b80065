"""Split fit / gradient accumulation timing: the fused step (ofx_dqn_fit_robust, all options off) against
ofx_dqn_grad + ofx_dqn_apply on the same gathered rows, lean form, one card.
  - 256 rows fused and 256 rows split at k = 1, alternating, in three rounds (the rounds show the run-to-run spread);
  - k x 256 rows accumulated (k ofx_dqn_grad + one ofx_dqn_apply) against one fused step of k * 256 rows, k = 4 and 16,
    each on a handle of its own, with the device memory the handle's workspace took (free memory before the first call
    minus free memory after the last; the handle keeps its workspace between calls).
Wall time of the calls, which end in the step's synchronisation; median (min, max).  The rows are gathered once from a
512-arena memory; targets are random.  Usage: python tools/accumulate_time.py [reps]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch    # before libofx.so is loaded; torch.cuda.mem_get_info reads the card's free memory

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.agents.policy_weights import synthetic

N, M, BATCH, SEED, ROWS = 512, 8, 8, 0x0F160071, 256
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30


def gather():
    """4096 real rows and their `state` maps on the device; they outlive the batch that gathered them"""
    b = ArenaBatch(N, M)
    b.replay_create(16, 0)
    b.spawn_random(SEED)
    ia, ip = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(10):
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.policy_explore(1.0, SEED, tick=t, collecting=True, iaction_ptr=ia.ptr, ipointer_ptr=ip.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, iaction_ptr=ia.ptr, ipointer_ptr=ip.ptr)
        b.replay_capture(t, None, ia.ptr, ip.ptr)
        b.step(actions_ptr=b._actions.ptr)
    slot, _ = b.replay_sample(7, 0, BATCH)
    rows, bp, _ = b.replay_gather_device(slot, BATCH)
    b.sync()
    n = N * BATCH
    assert (rows.download(b.TRANSITION_DTYPE, (n,))["ship"] >= 0).all()
    row_bytes = b.TRANSITION_DTYPE.itemsize
    b.close()
    return n, rows, bp, row_bytes


class Bench:
    def __init__(self, rows, bp, row_bytes, y, y2, w):
        self.rows, self.bp, self.row_bytes, self.y, self.y2 = rows, bp, row_bytes, y, y2
        z = np.zeros_like(w)
        self.w, self.m, self.v = (DeviceBuffer(w.nbytes).upload(a) for a in (w, z, z))
        self.step = 0

    def open(self):
        torch.cuda.synchronize()
        self.free0 = torch.cuda.mem_get_info()[0]
        self.b = ArenaBatch(1, M)
        self.acc = DeviceBuffer(4 * self.b.dqn_acc_floats())

    def close(self):
        """-> bytes the handle took since open() (its workspace; the small arena state included)"""
        self.b.sync()
        used = self.free0 - torch.cuda.mem_get_info()[0]
        self.acc.free()
        self.b.close()
        return used

    def fused(self, n):
        self.step += 1
        self.b.dqn_fit_robust(self.w, self.m, self.v, self.step, 1e-4, n, self.rows.ptr, self.bp.ptr, self.y.ptr, self.y2.ptr)

    def split(self, k):
        self.step += 1
        for i in range(k):
            o = i * ROWS
            self.b.dqn_grad(self.w, ROWS, self.rows.ptr + o * self.row_bytes, self.bp.ptr + o * 2 * 5000 * 4,
                            self.y.ptr + 4 * o, self.y2.ptr + 4 * o, self.acc, i == 0)
        self.b.dqn_apply(self.w, self.m, self.v, self.step, 1e-4, self.acc, 1.0 / k)

    def timed(self, fn, reps):
        for _ in range(3):
            fn()
        self.b.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts


def line(what, ts, extra=""):
    return "%-44s %8.3f ms  (min %.3f, max %.3f)%s" % (what, float(np.median(ts)), min(ts), max(ts), extra)


def main():
    n, rows, bp, row_bytes = gather()
    rs = np.random.RandomState(3)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    bench = Bench(rows, bp, row_bytes, y, y2, synthetic())
    out = ["%d gathered rows, lean fit, %d reps after 3 warm-up calls (large steps: %d reps)" % (n, REPS, max(5, REPS // 3))]
    bench.open()
    for r in range(3):
        a, s = [], []
        bench.timed(lambda: bench.fused(ROWS), 0), bench.timed(lambda: bench.split(1), 0)     # warm-up calls alone
        for _ in range(REPS):                                # alternating: a drift of the card hits both alike
            for fn, ts in ((lambda: bench.fused(ROWS), a), (lambda: bench.split(1), s)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        out.append(line("round %d: fused, 256 rows" % r, a))
        out.append(line("round %d: grad + apply (k = 1), 256 rows" % r, s, "  ratio %.3f" % (np.median(s) / np.median(a))))
    out.append("workspace after the 256-row steps: %.1f MB" % (bench.close() / 1e6))
    big = max(5, REPS // 3)
    for k in (4, 16):
        bench.open()
        ts = bench.timed(lambda: bench.split(k), big)
        ws = bench.close()
        out.append(line("%2d x 256 rows accumulated" % k, ts, "  workspace %.1f MB" % (ws / 1e6)))
        bench.open()
        tf = bench.timed(lambda: bench.fused(k * ROWS), big)
        wf = bench.close()
        out.append(line("one fused step of %d rows" % (k * ROWS), tf, "  workspace %.1f MB" % (wf / 1e6)))
        out.append("   accumulated / fused: time %.3f, workspace %.3f" % (np.median(ts) / np.median(tf), ws / wf))
    print("\n".join(out))


if __name__ == "__main__":
    main()
