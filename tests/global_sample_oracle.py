"""CPU restatement of the global sampling contract in include/ofx.h (ofx_replay_sample_global,
ofx_replay_update_priorities_list), on top of tests/per_oracle.py.  Plain Python floats are IEEE float64 with every
operation rounded on its own, which is what ofx_replay.hip computes under -ffp-contract=off: arenas and slots must match
exactly; the weights go through pow, the one inexact step."""
import bisect

import numpy as np

from oracle.pyoracle import philox
from tests import per_oracle

STREAM_GLOBAL = 5
GROUP = 256


def draw_int(r, n_inclusive):
    """ofx_draw_int: an integer in [0, n_inclusive] from one 32-bit word."""
    return (int(r) * (n_inclusive + 1)) >> 32


def strata(R, n):
    """The n integer ranges [j * R / n, (j + 1) * R / n) of the uniform mode."""
    return [(j * R // n, (j + 1) * R // n) for j in range(n)]


def exclusive_scan(v):
    out, run = [], 0
    for x in v:
        out.append(run)
        run += int(x)
    return out


def locate(off, idx):
    """Row idx of the (arena, oldest-first) sequence of eligible rows -> (arena, index among its eligible rows): the
    last arena whose exclusive offset is <= idx (an empty arena shares its offset with the next one and is passed)."""
    a = bisect.bisect_right(off, idx) - 1
    return a, idx - off[a]


def sample_uniform(v, skip, n_rows, seed, arena_base, draw):
    """v[a] eligible rows after skip[a] expired ones -> (arena [n], slot [n], n, R)."""
    R = int(sum(v))
    n = min(int(n_rows), R)
    arena, slot, off = [], [], exclusive_scan(v)
    for j, (lo, hi) in enumerate(strata(R, n) if n else []):
        r = philox(arena_base, j, draw, STREAM_GLOBAL, seed)
        a, i = locate(off, lo + draw_int(r[0], hi - lo - 1))
        arena.append(a)
        slot.append(skip[a] + i)
    return arena, slot, n, R


def group_scan(T):
    """Inclusive cross-arena prefix G of the arena totals T: sequential running sums inside groups of 256 arenas, the
    groups' last sums chained, G[a] = X_k + s_a."""
    G, X = [], 0.0
    for k0 in range(0, len(T), GROUP):
        s = 0.0
        for t in T[k0:k0 + GROUP]:
            s += float(t)
            G.append(X + s)
        X = X + s
    return G


def sample_prioritized(mass, skip, n_rows, beta, seed, arena_base, draw):
    """mass[a]: float32 masses of every row of arena a oldest first, the first skip[a] expired.
    -> (arena [n], slot [n], is_weight float32 [n] over its maximum, n, R)."""
    elig = [[float(x) for x in np.asarray(m, np.float32)[s:]] for m, s in zip(mass, skip)]
    v = [len(e) for e in elig]
    R = sum(v)
    n = min(int(n_rows), R)
    if n == 0:
        return [], [], np.zeros(0, np.float32), 0, R
    T = [per_oracle.prefix_chain(e)[1] for e in elig]
    G = group_scan(T)
    total = G[-1]
    last = max(a for a in range(len(v)) if v[a] > 0)
    chains = {}
    arena, slot, raw = [], [], []
    for j in range(n):
        r = philox(arena_base, j, draw, STREAM_GLOBAL, seed)
        U = int(r[0]) * 2.0 ** -32
        u = (j + U) / n * total
        a = bisect.bisect_right(G, u)                   # the first arena with G > u (G is monotone: group_scan)
        if a == len(G):
            a = last
        up = u - (G[a - 1] if a else 0.0)
        m = elig[a]
        if a not in chains:
            excl, t = per_oracle.prefix_chain(m)
            chains[a] = (per_oracle.chunk_bounds(len(m)), excl, excl[1:] + [t])
        chunks, excl, incl = chains[a]
        k = next((k for k, (lo, hi) in enumerate(chunks) if hi > lo and incl[k] > up), None)
        pick = len(m) - 1
        if k is not None:
            lo, hi = chunks[k]
            run, pick = 0.0, hi - 1
            for i in range(lo, hi):
                run += m[i]
                if excl[k] + run > up:
                    pick = i
                    break
        arena.append(a)
        slot.append(skip[a] + pick)
        raw.append((R * m[pick] / total) ** (-beta) if total > 0.0 else 1.0)
    w = np.array(raw, np.float32)
    if w.max() > 0:
        w = w / w.max()
    return arena, slot, w, n, R


def write_back(mass, mmax, arena, slot, lands, td, alpha, eps):
    """The list write-back with levelling.  mass[a] float arrays (oldest first), mmax [N], lands[j]: entry j names a row
    that still holds the gathered (tick_prev, ship).  Every entry that lands with finite errors raises mmax; of a run of
    adjacent entries naming one (arena, slot) the last such entry sets the mass; every mmax becomes the maximum."""
    mass = [np.array(m, np.float64) for m in mass]
    mmax = [float(x) for x in mmax]
    for j, (a, s) in enumerate(zip(arena, slot)):
        if not lands[j] or not np.isfinite(td[j]).all():
            continue
        m = float(np.float32(per_oracle.new_mass(td[j][0], td[j][1], alpha, eps)))
        mmax[a] = max(mmax[a], m)
        mass[a][s] = m                                  # entries in list order: the later one of a run overwrites
    return mass, [max(mmax)] * len(mmax)
