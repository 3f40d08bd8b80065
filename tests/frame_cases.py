"""Weights that put the heat map's maximum on its frame (the cases of tests/test_gpu_head_frame_argmax.py, which says how
they are built) and the name of a frame position.  A helper module (not collected)."""
import numpy as np

CASES = ("top", "bottom", "left", "right", "corner")


def frame_weights(case, seed):
    from oracle import pyoracle
    w, shapes = pyoracle.policy_init(seed, trained_like=True)
    rs = np.random.RandomState(seed + 1000)
    o, shp = shapes["upconv3.beta"]
    w[o:o + 8] = rs.uniform(0.5, 1.0, 8)
    o, shp = shapes["upconv3.kernel"]
    w[o:o + int(np.prod(shp))] *= 0.1
    o, shp = shapes["upconv4.kernel"]
    assert shp == (3, 3, 8, 1)
    k = np.zeros((3, 3, 8), np.float32)
    jit = lambda *s: rs.uniform(0.9, 1.1, s).astype(np.float32)
    if case == "top":
        k[0], k[1] = -3.0 * jit(3, 8), jit(3, 8)
    elif case == "bottom":
        k[2], k[1] = -3.0 * jit(3, 8), jit(3, 8)
    elif case == "left":
        k[:, 0], k[:, 1] = -3.0 * jit(3, 8), jit(3, 8)
    elif case == "right":
        k[:, 2], k[:, 1] = -3.0 * jit(3, 8), jit(3, 8)
    else:
        k[:] = -jit(3, 3, 8)
        k[1, 1] = 4.0 * jit(8)
    w[o:o + 72] = k.reshape(-1)
    return w


def where(y, x):
    names = []
    if (y in (0, 399)) and (x in (0, 399)):
        return ["corner"]
    if y == 0:
        names.append("top")
    if y == 399:
        names.append("bottom")
    if x == 0:
        names.append("left")
    if x == 399:
        names.append("right")
    return names
