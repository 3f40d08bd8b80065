"""CPU model (numpy) of what the sparse streaming trunk k_trunk12<., true> (ofighters_amd/csrc/ofx_trunk.hip) executes,
for the counters of ofx_policy_trunk_stats.  Test infrastructure; tests/test_trunk_sparse_model.py checks it in the CPU suite,
tests/test_gpu_trunk_default.py compares the kernel's counters with it.

Geometry of the kernel: the 400 x 400 one-bit maps (ship, laser) become p1 = pool(relu(conv1)), 200 x 200, made two adjacent
pixels ("a pair", 100 per row) per lane from the 4 x 6 bit window of the pair; an image is walked in 20 steps of 10 conv2
rows, a step making the p1 rows [pa, pb) new; conv2 runs on 63 M-tiles of 16 pixels per step, flat over 5 row pairs x 200
columns."""
import numpy as np

SIDE, P1, PAIRS, STEPS, TH, THREADS, NT = 400, 200, 100, 20, 10, 1024, 63


def unpack(ship_bits, laser_bits):
    """maps_host(MAP_BITS) (numpy.packbits order, [N][20000] uint8 each) -> bool [N][400][400], the OR of the two planes
    (the kernel ORs the windows of both channels)."""
    s = np.unpackbits(np.ascontiguousarray(ship_bits, np.uint8), axis=1).reshape(-1, SIDE, SIDE)
    l = np.unpackbits(np.ascontiguousarray(laser_bits, np.uint8), axis=1).reshape(-1, SIDE, SIDE)
    return (s | l).astype(bool)


def pair_marks(bits):
    """bool [N][400][400] -> bool [N][200][100]: pair pp of p1 row Y is marked when any bit is set in its window, image
    rows 2 Y - 1 .. 2 Y + 2 x columns 4 pp - 1 .. 4 pp + 4 (zero outside the image)."""
    bits = np.asarray(bits, bool)
    pad = np.pad(bits, ((0, 0), (1, 3), (1, 5)))
    out = np.zeros((bits.shape[0], P1, PAIRS), bool)
    for dr in range(4):
        for dc in range(6):
            out |= pad[:, dr:dr + SIDE:2, dc:dc + SIDE:4]
    return out


def step_rows(step):
    """(pa, pb): the p1 rows a step makes."""
    return (TH * step + 1 if step else 0), min(TH * step + TH + 1, P1)


def lane_map(nrow, npass):
    """The kernel's q -> (py, pp) map: for pass `npass` of a step with nrow new rows, (py, pp, valid) per thread [1024]:
    row-major, q = tid + 1024 npass, 64 consecutive pairs of one row per wave."""
    q = np.arange(THREADS) + THREADS * npass
    return q // PAIRS, q % PAIRS, q < nrow * PAIRS


def table_passes(marks):
    """(run, total) table passes of the images of marks [N][200][100]: a wave's pass runs when any of its pairs is marked;
    the counter is kept by lane 0 of every wave (a wave whose lane 0 has no pair has none at all)."""
    run = total = 0
    for step in range(STEPS):
        pa, pb = step_rows(step)
        for npass in range(2 if pb - pa > TH else 1):
            py, pp, valid = lane_map(pb - pa, npass)
            m = marks[:, np.minimum(pa + py, P1 - 1), pp] & valid              # [N][1024]
            busy = valid.reshape(16, 64)
            assert (busy[:, 0] == busy.any(axis=1)).all()
            total += marks.shape[0] * int(busy[:, 0].sum())
            run += int(m.reshape(-1, 16, 64).any(axis=2).sum())
    return run, total


def tiles_run(marks):
    """bool [N][20][63]: the M-tiles the GEMM phase runs.  Tile T of a step holds the pixels 16 T .. 16 T + 15 of the step's
    5 row pairs x 200 columns; its window is the columns x - 1 .. x + 16 of the four p1 rows 10 step - 1 + 2 rp .. + 3; a
    marked pair marks its two columns.  A tile on the zero padding - column 0 or 199, crossing into the next row pair, the
    image's first or last row pair - always runs; every other one runs when its window holds a mark."""
    cols = np.repeat(np.asarray(marks, bool), 2, axis=2)                         # [N][200][200]
    cols = np.pad(cols, ((0, 0), (1, 2), (0, 0)))                                # p1 rows -1 .. 201
    out = np.zeros((cols.shape[0], STEPS, NT), bool)
    for step in range(STEPS):
        for T in range(NT):
            P = 16 * T
            rp, x = divmod(P, P1)
            if x < 1 or x + 15 > P1 - 2 or P + 15 >= 5 * P1 or (step == 0 and rp == 0) or (step == STEPS - 1 and rp == 4):
                out[:, step, T] = True
            else:
                r0 = TH * step - 1 + 2 * rp + 1                                  # + 1: the padded row index
                out[:, step, T] = cols[:, r0:r0 + 4, x - 1:x + 17].any(axis=(1, 2))
    return out
