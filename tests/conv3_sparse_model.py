"""CPU model (numpy) of what the sparse streaming conv3 k_conv3_stream<., true> (ofighters_amd/csrc/ofx_trunk.hip) executes,
for the counters of ofx_policy_trunk_stats3.  Test infrastructure; tests/test_conv3_sparse_model.py checks it in the CPU
suite, tests/test_gpu_conv3_sparse.py compares the kernel's counters with it.

Geometry: k_trunk12<., true> marks every p2 pixel (100 x 100) written by a conv2 M-tile that ran - tile T of a step writes
the pooled pixels 8 T .. 8 T + 7 of the step's flat 5 rows x 100 columns; conv3 walks an image in 5 steps of 20 rows (10 row
pairs) and runs 63 M-tiles of 16 pixels per step, flat over 10 row pairs x 100 columns."""
import numpy as np

from tests import trunk_sparse_model as TM

P2, STEPS, TH, RP, NT = 100, 5, 20, 10, 63


def p2_marks(run2):
    """bool [N][20][63] (trunk_sparse_model.tiles_run: conv2's M-tiles that run) -> bool [N][100][100]: the p2 pixels that
    may differ from conv2's constant.  The half tile 62 of a step writes four pixels only."""
    run2 = np.asarray(run2, bool)
    assert run2.shape[1:] == (TM.STEPS, TM.NT)
    flat = np.repeat(run2, 8, axis=2)[:, :, :5 * P2]                             # [N][20][500]
    return flat.reshape(run2.shape[0], P2, P2)


def tiles_run(marks2):
    """bool [N][100][100] -> bool [N][5][63]: conv3's M-tiles that run.  Tile T of a step holds the pixels 16 T .. 16 T + 15
    of the step's 10 row pairs x 100 columns; its window is the columns x - 1 .. x + 16 of the four p2 rows
    20 step - 1 + 2 rp .. + 3.  A tile on the zero padding - column 0 or 99, crossing into the next row pair, the image's
    first or last row pair, the half tile at the step's end - always runs; every other one when its window holds a mark."""
    marks2 = np.asarray(marks2, bool)
    pad = np.pad(marks2, ((0, 0), (1, 1), (0, 0)))                               # p2 rows -1 .. 100
    out = np.zeros((marks2.shape[0], STEPS, NT), bool)
    for step in range(STEPS):
        for T in range(NT):
            P = 16 * T
            rp, x = divmod(P, P2)
            if x < 1 or x + 15 > P2 - 2 or P + 15 >= RP * P2 or (step == 0 and rp == 0) or (step == STEPS - 1 and rp == RP - 1):
                out[:, step, T] = True
            else:
                r0 = TH * step - 1 + 2 * rp + 1                                  # + 1: the padded row index
                out[:, step, T] = pad[:, r0:r0 + 4, x - 1:x + 17].any(axis=(1, 2))
    return out


def counts(bits):
    """bool [N][400][400] (trunk_sparse_model.unpack) -> (run, total) of ofx_policy_trunk_stats3 for one forward."""
    run2 = TM.tiles_run(TM.pair_marks(bits))
    run3 = tiles_run(p2_marks(run2))
    return int(run3.sum()), run3.shape[0] * STEPS * NT
