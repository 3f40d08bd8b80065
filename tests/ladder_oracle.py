"""The exploration ladder's law on the host, for tests/test_epsilon_ladder.py and tests/test_gpu_epsilon_ladder.py.

A ship of local arena a explores iff `collecting or u <= eps_a`, with eps_a formed from the call's epsilon and the arena's
exponent under the kernel's special cases (include/ofx.h, ofx_policy_epsilon_ladder): +inf never explores, whatever
`collecting` says; exponent 1 is epsilon itself, bit for bit; anything else is pow(epsilon, exponent) in float64.  The
draw itself - u and the random play - is oracle.pyoracle.policy_explore's, asked with eps_a as its epsilon.

The device's pow and glibc's may differ in the last bit.  u is a multiple of 2^-32, so `u <= eps_a` can only come out
differently where eps_a * 2^32 lies within an ulp of an integer: flip_distance() measures how far the inputs of a test
keep away from that, and the tests assert it before they compare anything.
"""
import math

import numpy as np


def arena_eps(epsilon, exponent):
    """eps_a, or None for a greedy arena."""
    if math.isinf(exponent):
        return None
    if exponent == 1.0:
        return float(epsilon)
    return math.pow(float(epsilon), float(exponent))


def flip_distance(epsilons, exponents):
    """The smallest distance of any eps_a * 2^32 from the nearest integer, over every epsilon and every arena that is not
    greedy and whose eps_a is neither 0 nor 1 (those are exact on both sides: pow(0, x > 0), pow(x, 0), pow(1, x))."""
    best = 1.0
    for eps in epsilons:
        for x in exponents:
            e = arena_eps(eps, x)
            if e is None or e in (0.0, 1.0):
                continue
            v = e * 4294967296.0
            best = min(best, abs(v - round(v)))
    return best


def explore(pyoracle, M, epsilon, exponents, seed, arena_base, tick, collecting=False):
    """The oracle's draw for every ship of the len(exponents) local arenas: (hit bool [N][M], play int32 [N][M][3] =
    (iaction, px, py) where hit)."""
    N = len(exponents)
    cfg = pyoracle.default_cfg(M)
    hit = np.zeros((N, M), bool)
    play = np.zeros((N, M, 3), np.int32)
    for a in range(N):
        e = arena_eps(epsilon, exponents[a])
        if e is None:
            continue                                   # greedy: always None, `collecting` included
        for i in range(M):
            r = pyoracle.policy_explore(cfg, e, seed, arena_base + a, i, tick, collecting)
            if r is not None:
                hit[a, i] = True
                play[a, i] = r
    return hit, play


def scalar(pyoracle, N, M, epsilon, seed, arena_base, tick, collecting=False):
    """The rule without a ladder: every arena at epsilon itself."""
    return explore(pyoracle, M, epsilon, np.ones(N), seed, arena_base, tick, collecting)


def expected(base_ia, base_ip, hit, play, mask=None):
    """(iaction [N][M], ipointer [N][M][2]) after the explore call: the random play where a selected ship explores, the
    base everywhere else."""
    sel = hit if mask is None else hit & (np.asarray(mask) != 0)
    ia, ip = np.array(base_ia, np.int32), np.array(base_ip, np.int32)
    ia[sel] = play[sel][:, 0]
    ip[sel] = play[sel][:, 1:]
    return ia, ip


# ---- the inputs of the explore tests: one ladder over the handle's own 40 arenas (36 rungs from exponent 1 to 8, then 4
# greedy arenas); the handle sits at arena_base 40, which keys the draws.  S = 320 ships cross a 256-thread block.
N, M, ARENA_BASE, EVAL, ALPHA, SEED = 40, 8, 40, 4, 7.0, 99
EPSILONS = (0.4, 0.9)
BAND = 8                                               # arenas per rung band of the hit counts: 64 ships


def ladder():
    from ofighters_amd.exploration import apex_exponents
    return apex_exponents(N, ALPHA, 0, N, eval_arenas=EVAL)


def band_hits(hit):
    """Exploring ships per band of BAND consecutive learning arenas (the last band is the partial one)."""
    L = N - EVAL
    return [int(hit[a:min(a + BAND, L)].sum()) for a in range(0, L, BAND)]
