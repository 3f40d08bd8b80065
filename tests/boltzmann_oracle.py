"""Boltzmann exploration on the host, in float64: the reference of tests/test_boltzmann.py and tests/test_gpu_boltzmann.py.

The law (include/ofx.h, ofx_policy_act_boltzmann): a Philox4x32-10 word r keyed by the seed gives w = (r + 0.5) / 2^32,
E = -ln(1 - w), g = -ln(E), a standard Gumbel variable; pixel (x, y) of ship i of global arena G takes word [x & 3] of
counter (G, i * (W*H/4) + (y*W + x) / 4, tick, stream 6), action k word [k] of counter (G, i, tick, stream 7).  The
choice is the first maximum in C order of fmaf(T, g, value) in float32: by the Gumbel-max identity a sample from
softmax(value / T).  T = tau * (float)eps_a in float32, eps_a the ladder's rate (tests/ladder_oracle.py arena_eps).

Philox is oracle.pyoracle.philox, the project's one restatement of the generator.  It answers one counter per call
through ctypes; a 400x400 map needs 40 000 of them and the GPU tests need dozens of maps, so whole maps are drawn by
`philox_words`, the same ten rounds on numpy arrays.  It is not a second definition: tests/test_boltzmann.py holds it to
pyoracle.philox word for word, and `noise_map(..., scalar=True)` draws through pyoracle.philox alone.

A device choice c is ACCEPTED iff ref[c] >= max(ref) - tol, ref the perturbed map formed here from the device's own
stored heat map and tol = 2 T GUMBEL_ABS_ERR + 4 ulp_f32(max |ref|): the device evaluates g in float32.
"""
import math

import numpy as np

from oracle import pyoracle
from tests import ladder_oracle

STREAM_PTR, STREAM_ACT = 6, 7
# twice the largest |g_device - g_float64| measured with ofx_policy_gumbel over the edge words and 2^20 Philox words on
# the MI355X (profiles/r19_boltzmann.txt); the contract's own bound is 1e-4
GUMBEL_MEASURED = 9.276e-6
GUMBEL_ABS_ERR = 2 * GUMBEL_MEASURED
GUMBEL_BOUND = 1e-4

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


def philox_words(seed, c0, c1, c2, c3):
    """pyoracle.philox(c0, c1, c2, c3, seed) for arrays of counters (broadcast together): uint32 [..., 4]."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & _LO, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & _LO]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def gumbel(r):
    """g of Philox words r, float64 (log1p: 1 - w is never rounded)."""
    w = (np.asarray(r, dtype=np.float64) + 0.5) / 4294967296.0
    return -np.log(-np.log1p(-w))


def noise_map(seed, G, i, tick, W=400, H=400, scalar=False):
    """g of every pixel of ship i of global arena G at `tick`: float64 [H][W].  tick may be an array [K]: [K][H][W]."""
    assert (W * H) % 4 == 0 and W % 4 == 0
    blocks = i * (W * H // 4) + np.arange(W * H // 4, dtype=np.int64)
    if scalar:
        r = np.stack([pyoracle.philox(G, int(b), int(tick), STREAM_PTR, seed) for b in blocks])
        return gumbel(r).reshape(H, W)
    t = np.asarray(tick, dtype=np.int64)
    r = philox_words(seed, G, blocks, t[..., None], STREAM_PTR)        # [..., W*H/4, 4]
    return gumbel(r).reshape(t.shape + (H, W))


def action_noise(seed, G, i, tick):
    """(g0, g1) of the action head; tick may be an array [K]: float64 [K][2]."""
    if np.ndim(tick) == 0:
        return gumbel(pyoracle.philox(G, i, int(tick), STREAM_ACT, seed)[:2])
    return gumbel(philox_words(seed, G, i, np.asarray(tick, dtype=np.int64), STREAM_ACT)[..., :2])


def temperatures(tau, epsilon, exponents=None, n=None):
    """float32 [N]: T[a] = float32(tau) * float32(eps_a); exponent 1 (or no ladder) leaves epsilon bit for bit, +inf
    gives 0."""
    if exponents is None:
        exponents = np.ones(n)
    out = np.zeros(len(exponents), np.float32)
    for a, x in enumerate(exponents):
        e = ladder_oracle.arena_eps(epsilon, float(x))
        out[a] = np.float32(tau) * np.float32(0.0 if e is None else e)
    return out


def perturbed(values, T, g):
    """fmaf(T, g, values) rounded to float32, from the float64 g; T == 0: the values themselves (no noise is drawn)."""
    v = np.asarray(values, dtype=np.float32)
    if float(T) == 0.0:
        return v.copy()
    return (np.float64(np.float32(T)) * np.asarray(g, np.float64) + v.astype(np.float64)).astype(np.float32)


def choose_pointer(heat, T, g):
    """(px, py): the first maximum in C order of the perturbed map."""
    ref = perturbed(heat, T, g)
    k = int(np.argmax(ref))
    return k % ref.shape[1], k // ref.shape[1]


def choose_action(act, T, g01):
    """1 iff the perturbed act[1] beats the perturbed act[0] strictly."""
    p = perturbed(np.asarray(act, np.float32), T, g01)
    return int(p[1] > p[0])


def ulp_f32(x):
    return float(np.spacing(np.float32(abs(float(x)))))


def tolerance(ref, T):
    return 2.0 * float(T) * GUMBEL_ABS_ERR + 4.0 * ulp_f32(np.abs(ref).max())


def accepted(ref, flat_index, T):
    """The acceptance rule for near-ties: the device's choice is within `tolerance` of the reference's maximum."""
    ref = np.asarray(ref)
    return float(ref.reshape(-1)[flat_index]) >= float(ref.max()) - tolerance(ref, T)


def softmax(values, T):
    z = np.asarray(values, np.float64).reshape(-1) / float(T)
    p = np.exp(z - z.max())
    return p / p.sum()


def edge_words():
    """0, 1, 2^32 - 1 and 2^k, 2^k +- 1 for every k: uint32, unique."""
    w = {0, 1, 0xFFFFFFFF}
    for k in range(32):
        w.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v <= 0xFFFFFFFF)
    return np.array(sorted(w), np.uint32)
