"""Where the sparse trunk stops paying: the policy forward (one policy ship per arena, so that the trunk is a large part
of it) on arenas late in an episode of turret bots - every ship shooting on every tick, the laser map as full as the game
makes it - with the dense trunk (OFX_OPT_TRUNK_SPARSE = 0) and with the default, interleaved, plus the executed fractions
of the counters.  Run it under `rocprofv3 --kernel-trace --stats` to get k_trunk12<0, false> and k_trunk12<0, true> as
kernel averages of the same maps (the rollout itself runs no forward).

usage: python tools/trunk_saturated.py [arenas=4096] [ticks=150] [reps=10]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.agents.policy_weights import synthetic
    N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 150
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    M = 8
    b = ArenaBatch(N, M)
    b.spawn_random(7)
    for t in range(ticks):
        b.bot_actions(["turret"] * M, 7, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    w = np.ascontiguousarray(synthetic(), np.float32)
    dw = DeviceBuffer(w.nbytes).upload(w)
    b.policy_pin_weights(dw.ptr)
    mask = np.zeros((N, M), np.uint8)
    mask[:, 0] = 1
    dm = DeviceBuffer(mask.nbytes).upload(mask)
    sm, lm = (np.unpackbits(x[:256]) for x in b.maps_host(nat.MAP_BITS))    # the first 256 arenas
    print("arenas %d, tick %d, 8 turret bots: set cells %.2f %% (ships) %.2f %% (lasers), lasers per arena %.1f"
          % (N, ticks, 100 * float((sm != 0).mean()), 100 * float((lm != 0).mean()), float(b.get(nat.F_N_LASERS).mean())))
    del sm, lm

    def forward_ms():
        b.sync()
        t0 = time.perf_counter()
        b.policy_forward(dw.ptr, dm.ptr)
        b.sync()
        return 1e3 * (time.perf_counter() - t0)

    b.set_option(nat.OPT_TRUNK_SPARSE, 1)
    forward_ms()
    b.policy_trunk_stats()
    forward_ms()
    run, total, trun, ttotal = b.policy_trunk_stats()
    print("executed: %.1f %% of conv2's M-tiles, %.1f %% of the table passes" % (100 * run / total, 100 * trun / ttotal))
    ms = {0: [], 1: []}
    for _ in range(reps):
        for opt in (0, 1):
            b.set_option(nat.OPT_TRUNK_SPARSE, opt)
            forward_ms()
            ms[opt].append(forward_ms())
    for opt, name in ((0, "dense (option 0)"), (1, "sparse")):
        print("forward, %-17s median %.3f ms  min %.3f  max %.3f" % (name, np.median(ms[opt]), min(ms[opt]), max(ms[opt])))
    b.close()


if __name__ == "__main__":
    main()
