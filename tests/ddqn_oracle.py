"""CPU restatement of the target network / Double DQN contract in include/ofx.h (ofx_dqn_targets_double,
ofx_policy_blend_weights).  numpy float32 throughout: every numpy operation on float32 arrays rounds on its own, which is
what ofx_train.hip computes under -ffp-contract=off, so the results must match exactly.  The TD arithmetic itself is
tests/td_oracle.py's."""
import numpy as np

from tests import td_oracle

_F = np.float32


def targets_double(rows, gamma, ret, disc, iaction_online, act_target, probe_target):
    """rows: the gathered transitions (engine.ArenaBatch.TRANSITION_DTYPE; ship, reward and done are read);
    iaction_online [n]: the online network's arg-max action on next_state; act_target [n][2]: the target network's
    action values on next_state; probe_target [n]: the target network's heat map at the online network's ipointer.
    ret = disc = None: y = (float)reward + gamma * v * live, else y = ret + disc * v (gamma ignored); the product is
    rounded, then the sum.  Padding rows (ship < 0) give zeros.  Returns (y_act, y_ptr) float32 [n]."""
    if (ret is None) != (disc is None):
        raise ValueError("targets_double: pass ret and disc together")
    n = len(rows)
    act = np.asarray(act_target, _F).reshape(n, 2)
    sel = (np.asarray(iaction_online).reshape(n) != 0).astype(np.intp)
    v_act = act[np.arange(n), sel]                               # evaluation of the online selection
    return td_oracle.targets(rows, gamma, v_act, np.asarray(probe_target, _F).reshape(n), ret, disc)


def blend(dst, src, tau):
    """ofx_policy_blend_weights: c * dst + tau * src with c = 1 - tau formed once in float32, both products rounded,
    then the sum; tau == 1 is a copy of src (whatever dst holds), tau == 0 leaves dst.  Returns a new float32 array."""
    dst, src, t = np.asarray(dst, _F), np.asarray(src, _F), _F(tau)
    if not (t >= 0 and t <= 1):
        raise ValueError("blend: tau must lie in [0, 1], got %r" % (tau,))
    if t == 1:
        return src.copy()
    if t == 0:
        return dst.copy()
    c = _F(1) - t
    out = c * dst + t * src
    assert out.dtype == _F
    return out
