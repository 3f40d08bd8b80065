"""CPU restatement of the prioritized replay contract in include/ofx.h (ofx_replay_sample_prioritized,
ofx_replay_window_weights, ofx_replay_update_priorities).  Plain Python floats are IEEE float64 with every operation
rounded on its own, which is what ofx_replay.hip computes under -ffp-contract=off: the slots must match exactly."""
import numpy as np

from oracle.pyoracle import philox

STREAM_PER = 4
CHUNKS = 64


def chunk_bounds(valid):
    """The 64 contiguous chunks of ceil(valid / 64) eligible rows: [(lo, hi)], empty ones at the end."""
    cs = -(-valid // CHUNKS)
    return [(min(k * cs, valid), min(k * cs + cs, valid)) for k in range(CHUNKS)]


def prefix_chain(mass):
    """(excl [64], total): the chunk totals summed row by row, chained in chunk order."""
    m = [float(x) for x in np.asarray(mass, np.float32)]
    excl, acc = [], 0.0
    for lo, hi in chunk_bounds(len(m)):
        t = 0.0
        for i in range(lo, hi):
            t += m[i]
        excl.append(acc)
        acc += t
    return excl, acc


def row_prefixes(mass):
    """Inclusive prefix of every eligible row as the contract defines it: excl[chunk] + running sum inside the chunk."""
    m = [float(x) for x in np.asarray(mass, np.float32)]
    excl, _ = prefix_chain(m)
    out = []
    for k, (lo, hi) in enumerate(chunk_bounds(len(m))):
        run = 0.0
        for i in range(lo, hi):
            run += m[i]
            out.append(excl[k] + run)
    return out


def sample(mass, batch, beta, seed, global_arena, draw):
    """One arena: mass = float32 masses of its ELIGIBLE rows, oldest first.  Returns (rows drawn as indices into mass,
    raw IS weights as float32), n = min(batch, len(mass)) of each."""
    m = [float(x) for x in np.asarray(mass, np.float32)]
    valid = len(m)
    n = min(batch, valid)
    if n == 0:
        return [], np.zeros(0, np.float32)
    chunks = chunk_bounds(valid)
    excl, total = prefix_chain(m)
    incl = excl[1:] + [total]
    picks, weights = [], []
    for j in range(n):
        r = philox(global_arena, j, draw, STREAM_PER, seed)
        U = int(r[0]) * 2.0 ** -32
        u = (j + U) / n * total
        k = next((k for k, (lo, hi) in enumerate(chunks) if hi > lo and incl[k] > u), None)
        pick = valid - 1
        if k is not None:
            lo, hi = chunks[k]
            run, pick = 0.0, hi - 1
            for i in range(lo, hi):
                run += m[i]
                if excl[k] + run > u:
                    pick = i
                    break
        picks.append(pick)
        weights.append((valid * m[pick] / total) ** (-beta) if total > 0.0 else 1.0)
    return picks, np.array(weights, np.float32)


def sample_arena(mass_all, skip, batch, beta, seed, global_arena, draw):
    """mass_all: every row of the arena oldest first, the first `skip` expired.  -> (slot [batch] with -1 pads,
    n, is_weight [batch] with 0 in pads), the layout of ofx_replay_sample_prioritized."""
    picks, w = sample(np.asarray(mass_all, np.float32)[skip:], batch, beta, seed, global_arena, draw)
    slot = np.full(batch, -1, np.int32)
    iw = np.zeros(batch, np.float32)
    slot[:len(picks)] = np.asarray(picks, np.int32) + skip
    iw[:len(picks)] = w
    return slot, len(picks), iw


def window_weights(is_weight, n_sampled, first, max_rows):
    """The packed (arena, j) window of ofx_replay_gather_valid, divided by its maximum (float32)."""
    packed = np.concatenate([is_weight[a, :n] for a, n in enumerate(n_sampled)]).astype(np.float32)
    win = packed[first:first + max_rows]
    return win / win.max() if len(win) and win.max() > 0 else win


def new_mass(e1, e2, alpha, eps):
    """m = p^alpha with p = |e1| + |e2| + eps summed in float32, the power in float64 (the device's powf is the check)."""
    p = np.float32(np.float32(abs(np.float32(e1)) + abs(np.float32(e2))) + np.float32(eps))
    return float(p) ** float(np.float32(alpha))
