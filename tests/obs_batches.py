"""Host-side builders of stored-observation batches for tests/test_gpu_forward_obs.py.  Test infrastructure, numpy only.

The layout is the one ofx_replay_gather documents (include/ofx.h): bits[n][2 (ship, laser)][W*H/32] uint32, pixel
p = y * W + x stored as bit (p & 7) of byte p >> 3 of its map - numpy.unpackbits(bitorder='little') on a little-endian
host.  tests/test_obs_batches.py checks these builders in the CPU suite."""
import numpy as np

SIDE = 400
PIXELS = SIDE * SIDE
WORDS = PIXELS // 32

# maps an arena never produces (name -> what the two planes hold)
PATTERNS = ("zero", "ones", "dense", "half", "frame", "ship_only", "laser_only")


def pack_maps(x):
    """bool / 0-1 maps [n][2][400][400] -> uint32 [n][2][5000] in the stored layout."""
    x = np.asarray(x)
    n = x.shape[0]
    assert x.shape == (n, 2, SIDE, SIDE)
    return np.packbits(x.reshape(n, 2, PIXELS).astype(bool), axis=-1, bitorder="little").view(np.uint32)


def unpack_maps(bits):
    """uint32 [n][2][5000] -> uint8 [n][2][400][400]."""
    bits = np.ascontiguousarray(bits, np.uint32)
    n = bits.shape[0]
    assert bits.shape == (n, 2, WORDS)
    return np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(n, 2, SIDE, SIDE)


def pattern_maps(name, n, rs):
    """n observations of one pattern as bool [n][2][400][400]; rs = numpy RandomState (the random patterns differ per
    observation, the fixed ones repeat)."""
    x = np.zeros((n, 2, SIDE, SIDE), bool)
    if name == "zero":
        pass
    elif name == "ones":
        x[:] = True
    elif name == "dense":                   # no empty bit window anywhere
        x[:, 0] = rs.uniform(size=(n, SIDE, SIDE)) < 0.3
        x[:, 1] = rs.uniform(size=(n, SIDE, SIDE)) < 0.05
    elif name == "half":                    # left half of the ship map dense, bottom half of the laser map sparse
        x[:, 0, :, :SIDE // 2] = rs.uniform(size=(n, SIDE, SIDE // 2)) < 0.3
        x[:, 1, SIDE // 2:, :] = rs.uniform(size=(n, SIDE // 2, SIDE)) < 0.02
    elif name == "frame":                   # only the one-pixel frame of both maps
        x[:, :, [0, SIDE - 1], :] = True
        x[:, :, :, [0, SIDE - 1]] = True
    elif name == "ship_only":               # one map dense, the other empty
        x[:, 0] = rs.uniform(size=(n, SIDE, SIDE)) < 0.3
    elif name == "laser_only":
        x[:, 1] = rs.uniform(size=(n, SIDE, SIDE)) < 0.3
    else:
        raise ValueError("unknown pattern %r" % (name,))
    return x


def sweep_pixels(k):
    """Observation k of the sweep batch: ((ship y, ship x), (laser y, laser x))."""
    return (k, (7 * k + 3) % SIDE), ((11 * k + 5) % SIDE, k)


def sweep_bits():
    """400 observations, each with exactly one ship bit and one laser bit (sweep_pixels), written bit by bit into the
    stored layout (not through pack_maps): a lone non-constant neighbourhood on every row and every column of both maps."""
    b = np.zeros((SIDE, 2, PIXELS // 8), np.uint8)
    for k in range(SIDE):
        for plane, (y, x) in enumerate(sweep_pixels(k)):
            p = y * SIDE + x
            b[k, plane, p >> 3] |= np.uint8(1 << (p & 7))
    return b.view(np.uint32)


def frame_probes():
    """(x, y) probes on and next to the heat map's frame: the four corners, two points on every edge, and the two
    diagonal neighbours of opposite corners."""
    e = SIDE - 1
    corners = [(0, 0), (e, 0), (0, e), (e, e)]
    edges = [(1, 0), (e - 1, 0), (137, e), (e - 1, e), (0, 1), (0, 262), (e, e - 1), (e, 91)]
    return corners, edges, [(1, 1), (e - 1, e - 1)]
