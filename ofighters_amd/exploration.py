"""Per-arena exploration: the Ape-X ladder and greedy evaluation arenas (opt-in; Horgan et al. 2018).

Ape-X gives every actor its own exploration rate, eps_i = eps^(1 + alpha * i / (L - 1)) for actor i of L, so that the
memory holds near-greedy and strongly exploring experience at the same time.  Here an arena is an actor.  The library
takes one EXPONENT per local arena (ofx_policy_epsilon_ladder): the rate follows whatever schedule the trainer's epsilon
runs through, and an exponent of +inf makes an arena greedy - it plays the current weights and never explores.

Both functions are keyed by the GLOBAL arena id g = arena_base + a, like the counter RNG, so any sharding of the same
run gets the same ladder and the same groups.  Host arithmetic only: nothing here touches the device.
"""
import math

import numpy as np


def _integer(name, v, lo=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError("%s must be an integer, got %r" % (name, v))
    if lo is not None and v < lo:
        raise ValueError("%s must be >= %d, got %r" % (name, lo, v))
    return int(v)


def boltzmann_pair(v):
    """TrainingRollout's `boltzmann` argument: None (off) or a pair (tau_act, tau_ptr) of finite numbers >= 0, returned
    as a tuple of floats that float32 can hold.  ValueError naming `boltzmann` for anything else."""
    if v is None:
        return None
    if isinstance(v, (str, bytes)) or not hasattr(v, "__len__") or len(v) != 2:
        raise ValueError("boltzmann must be None or a pair (tau_act, tau_ptr), got %r" % (v,))
    out = []
    for name, x in zip(("tau_act", "tau_ptr"), v):
        if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
            raise ValueError("boltzmann: %s must be a number, got %r" % (name, x))
        x = float(x)
        if not (0.0 <= x <= float(np.finfo(np.float32).max)):   # NaN fails both comparisons
            raise ValueError("boltzmann: %s must be finite and >= 0, got %r" % (name, x))
        out.append(x)
    return tuple(out)


def _shard(total_arenas, arena_base, n, eval_arenas):
    total = _integer("total_arenas", total_arenas, 1)
    base = _integer("arena_base", arena_base, 0)
    n = _integer("n", n, 1)
    k = _integer("eval_arenas", eval_arenas)
    if not (0 <= k < total):
        raise ValueError("eval_arenas must be in [0, total_arenas = %d), got %r" % (total, eval_arenas))
    if base + n > total:
        raise ValueError("arenas [%d, %d) lie outside a run of total_arenas = %d" % (base, base + n, total))
    return total, base, n, k


def apex_exponents(total_arenas, alpha, arena_base, n, eval_arenas=0):
    """float64 [n]: the exponents of local arenas 0 .. n-1 of the shard that starts at global arena `arena_base`.

    With L = total_arenas - eval_arenas learning arenas, global arena g < L gets 1 + alpha * g / (L - 1) (1.0 when
    L == 1) and the last `eval_arenas` global arenas get +inf.  alpha = 0: every learning arena explores at epsilon
    itself.  ValueError for alpha < 0 or NaN, eval_arenas outside [0, total_arenas), a bool or a non-integer count."""
    total, base, n, k = _shard(total_arenas, arena_base, n, eval_arenas)
    if isinstance(alpha, (bool, np.bool_)) or not isinstance(alpha, (int, float, np.integer, np.floating)):
        raise ValueError("alpha must be a number, got %r" % (alpha,))
    alpha = float(alpha)
    if math.isnan(alpha) or math.isinf(alpha) or alpha < 0:
        raise ValueError("alpha must be finite and >= 0, got %r" % (alpha,))
    L = total - k
    g = base + np.arange(n, dtype=np.int64)
    expo = np.ones(n, np.float64) if L == 1 else 1.0 + alpha * g.astype(np.float64) / float(L - 1)
    expo[g >= L] = np.inf
    return expo


def score_groups(total_arenas, arena_base, n, bands, eval_arenas):
    """int32 [n]: the score group of every local arena.  The L = total_arenas - eval_arenas learning arenas are cut into
    `bands` contiguous bands by global id (band b holds the ids g with g * bands // L == b: equal sizes when bands
    divides L, else sizes that differ by at most one); the evaluation arenas, if any, form one last group `bands`.
    ValueError unless 1 <= bands <= L."""
    total, base, n, k = _shard(total_arenas, arena_base, n, eval_arenas)
    bands = _integer("bands", bands, 1)
    L = total - k
    if bands > L:
        raise ValueError("bands must be <= the %d learning arenas, got %d" % (L, bands))
    g = base + np.arange(n, dtype=np.int64)
    grp = (g * bands) // L
    grp[g >= L] = bands
    return grp.astype(np.int32)


def n_groups(bands, eval_arenas):
    """How many groups score_groups numbers: the bands and, with evaluation arenas, their group."""
    return int(bands) + (1 if eval_arenas else 0)
