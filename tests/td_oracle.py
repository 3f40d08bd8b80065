"""The TD target arithmetic of k_dqn_targets (ofx_train.hip), stated once in exact float32: what ofx_dqn_targets, _nstep,
_double and _soft compute from their two bootstrap values.  numpy float32 throughout: every numpy operation on float32
arrays rounds on its own, which is what ofx_train.hip computes under -ffp-contract=off, so the results must match exactly.
tests/ddqn_oracle.py and tests/nstep_oracle.py select their bootstrap values and call this; tests/soft_oracle.py is the
float64 statement of the soft values and stays apart."""
import numpy as np

_F = np.float32


def targets(rows, gamma, v_act, v_ptr, ret=None, disc=None, bonus_act=None, bonus_ptr=None):
    """rows: the gathered transitions (engine.ArenaBatch.TRANSITION_DTYPE; ship, reward and done are read), or None in
    the n-step form for rows known to hold no padding; v_act / v_ptr [n]: the bootstrap values of the two heads.
    ret = disc = None: y = ((float)reward [+ bonus]) + (gamma * v) * live with live = int(not done); bonus_act / bonus_ptr
    [n] (the Munchausen term, already scaled and clipped) join the reward first, in a rounding of their own.  Else
    y = ret + disc * v (gamma and the bonus do not enter).  The product is rounded, then the sum.  Padding rows
    (ship < 0) give zeros.  Returns (y_act, y_ptr) float32 [n]."""
    if (ret is None) != (disc is None):
        raise ValueError("targets: pass ret and disc together")
    if (bonus_act is None) != (bonus_ptr is None) or (bonus_act is not None and ret is not None):
        raise ValueError("targets: the bonus takes both heads and the one-step form")
    if rows is None and ret is None:
        raise ValueError("targets: the one-step form reads the rows")
    v = [np.asarray(x, _F).reshape(-1) for x in (v_act, v_ptr)]
    if ret is None:
        live = np.where(rows["done"] != 0, _F(0), _F(1))
        g = _F(gamma)
        base = [rows["reward"].astype(_F)] * 2
        if bonus_act is not None:
            base = [base[0] + np.asarray(bonus_act, _F), base[1] + np.asarray(bonus_ptr, _F)]
        y = [r + (g * x) * live for r, x in zip(base, v)]
    else:
        ret, disc = np.asarray(ret, _F), np.asarray(disc, _F)
        y = [ret + disc * x for x in v]
    if rows is not None:
        pad = rows["ship"] < 0
        y = [np.where(pad, _F(0), x) for x in y]
    assert y[0].dtype == _F and y[1].dtype == _F
    return y[0], y[1]
