"""CPU restatement of the n-step returns contract in include/ofx.h (ofx_replay_gather_nstep, ofx_dqn_targets_nstep).
Plain Python floats are IEEE float64 with every operation rounded on its own, which is what ofx_replay.hip computes under
-ffp-contract=off: ret and disc must match exactly."""
import numpy as np

from tests import td_oracle

# the composite row takes these fields from the chain's last row, every other one from the sampled row
FROM_END = ("tick_next", "frame_next", "head_next", "done")
REASONS = ("full", "done", "restart", "head")


def successor(rows, k):
    """Index of the row of the same ship whose tick_prev is rows[k]'s tick_next, or None (the contract: unique)."""
    hit = np.flatnonzero((rows["ship"] == rows["ship"][k]) & (rows["tick_prev"] == rows["tick_next"][k]))
    assert len(hit) <= 1, "two rows of ship %d chain from lock-step %d" % (rows["ship"][k], rows["tick_next"][k])
    return int(hit[0]) if len(hit) else None


def chain(rows, slot, nstep, gamma):
    """One arena's rows oldest first (the ofx_replay_rows_host layout, engine.ArenaBatch.TRANSITION_DTYPE), the sampled
    row's oldest-first index, nstep, gamma (a float32 argument of the C call) -> dict:
      row      the composite row (a copy)
      ticks    (tick of its state frame, tick of its next-state frame)
      ret      float32 discounted return, disc float32 bootstrap discount
      L        chain length, idx the chain's oldest-first indices
      reason   'done' (the last row has done != 0), 'full' (L == nstep), 'restart' (the ship has a later row that does
               not chain: an episode restart in between) or 'head' (the ship has no later row yet)"""
    g = float(np.float32(gamma))
    acc, p = 0.0, 1.0
    idx = [int(slot)]
    while True:
        r = rows[idx[-1]]
        acc += p * float(int(r["reward"]))
        p *= g
        if r["done"]:
            reason = "done"
            break
        if len(idx) == nstep:
            reason = "full"
            break
        nxt = successor(rows, idx[-1])
        if nxt is None:
            later = bool((rows["ship"][idx[-1] + 1:] == r["ship"]).any())
            reason = "restart" if later else "head"
            break
        idx.append(nxt)
    end = rows[idx[-1]]
    row = rows[idx[0]:idx[0] + 1].copy()[0]
    for f in FROM_END:
        row[f] = end[f]
    disc = np.float32(0.0) if end["done"] else np.float32(p)
    return dict(row=row, ticks=(int(row["tick_prev"]), int(row["tick_next"])), ret=np.float32(acc), disc=disc,
                L=len(idx), idx=idx, reason=reason)


def targets(ret, disc, act_next, ptr_max):
    """ofx_dqn_targets_nstep's arithmetic in float32 (tests/td_oracle.py): the product rounded, then the sum.
    act_next [n][2], ptr_max [n]."""
    act = np.asarray(act_next, np.float32)
    return td_oracle.targets(None, None, np.maximum(act[:, 0], act[:, 1]), ptr_max, ret, disc)
