"""float64 restatement of the soft and Munchausen targets (include/ofx.h, "soft and Munchausen targets").  numpy only;
a helper module (not collected).

The reference for ptr_soft / ptr_mass is the float64 log-sum-exp over the float32 heat map the call itself wrote, so the
reduction is measured apart from the forward's own error.  The reference for ofx_dqn_targets_soft is the float64
evaluation of the header's formulas on the float32 outputs of ofx_policy_forward_obs_soft for the same bits.

Measured on the MI355X (profiles/r21_soft_targets.txt, section 1) over the cases of tests/test_gpu_soft_targets.py
(tests 3 and 4: 9 observations x 5 temperatures under synthetic(7), 9 x 5 frame cases at T = 0.03): the largest relative
error of ptr_mass, 2.46e-7, and the largest part of |ptr_soft - ref| that 4 ulp(ref) does not cover, in units of T: none
- the largest error was 1.8 ulp(ref), since T ln Z inherits Z's relative error times T and the sum's last rounding is
half an ulp.  The tests allow twice the measured value and never more than the contract's bound.  Twice a measured 0 is
0: the ptr_soft tests allow exactly 4 ulp(ref), the T part of the contract is never drawn on, and the factor 2 between
the measured 1.84 ulp and those 4 ulp is the whole allowance."""
import numpy as np

MASS_REL_CONTRACT = 1e-4            # |ptr_mass - ref| <= 1e-4 ref
SOFT_T_CONTRACT = 1e-4              # |ptr_soft - ref| <= 1e-4 T + 4 ulp(ref)
MASS_REL_ERR = 2.46e-7              # measured: profiles/r21_soft_targets.txt
SOFT_T_ERR = 0.0                    # measured, in units of T, beyond the 4 ulp(ref): the same file
TARGET_REL = 2e-6                   # ofx_dqn_targets_soft: 2e-6 * max(1, |reward| + |alpha * clip| + |V|)


def mass_bound():
    return min(2.0 * MASS_REL_ERR, MASS_REL_CONTRACT)


def soft_bound(T, ref):
    """The allowed |ptr_soft - ref| at temperature T: min(2 x measured, contract) T + 4 ulp(ref) in float32."""
    ulp = np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)
    return min(2.0 * SOFT_T_ERR, SOFT_T_CONTRACT) * float(T) + 4.0 * ulp


def lse(values, T):
    """(soft value, mass, maximum) of `values` (any shape, reduced over all of it) at temperature T > 0, in float64:
    mass = sum exp((v - max) / T), soft = max + T ln mass."""
    v = np.asarray(values, np.float64).reshape(-1)
    m = v.max()
    z = np.exp((v - m) / float(T)).sum()
    return m + float(T) * np.log(z), z, m


def soft_rows(heat, T):
    """lse per row of heat [n][...]: (soft [n], mass [n]) float64; T == 0: the maxima and ones."""
    heat = np.asarray(heat)
    n = heat.shape[0]
    if T == 0:
        return heat.reshape(n, -1).max(axis=1).astype(np.float64), np.ones(n)
    out = [lse(heat[i], T) for i in range(n)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def soft_act(act, T):
    """The two-action soft value: max(a0, a1) + T log1p(exp(-|a0 - a1| / T)), T == 0: the maximum.  act [n][2]."""
    a = np.asarray(act, np.float64).reshape(-1, 2)
    m = a.max(axis=1)
    if T == 0:
        return m
    return m + float(T) * np.log1p(np.exp(-np.abs(a[:, 0] - a[:, 1]) / float(T)))


def munchausen_term(q, v, alpha, clip):
    """alpha * clamp(q - v, clip, 0)."""
    return float(alpha) * np.clip(np.asarray(q, np.float64) - np.asarray(v, np.float64), float(clip), 0.0)


def targets(rows, gamma, ret, disc, tau_act, act_next, soft_next, alpha=0.0, clip=0.0, act_prev=None, probe_prev=None,
            soft_prev=None):
    """(y_act, y_ptr) float64 [n] of ofx_dqn_targets_soft.  rows: gathered transitions (ship, reward, done, iaction are
    read); act_next [n][2] and soft_next [n] (= ptr_soft at tau_ptr) of next_state; with alpha > 0 also act_prev [n][2],
    probe_prev [n] (the heat value at the row's pointer) and soft_prev [n] of state.  ret / disc given: the n-step form
    y = ret + disc * V (gamma is ignored; no Munchausen term).  Padding rows (ship < 0) give zeros."""
    if (ret is None) != (disc is None):
        raise ValueError("targets: pass ret and disc together")
    if alpha > 0 and ret is not None:
        raise ValueError("targets: the Munchausen term takes the one-step form")
    n = len(rows)
    v_act = soft_act(act_next, tau_act)
    v_ptr = np.asarray(soft_next, np.float64).reshape(n)
    if ret is not None:
        y_act = np.asarray(ret, np.float64) + np.asarray(disc, np.float64) * v_act
        y_ptr = np.asarray(ret, np.float64) + np.asarray(disc, np.float64) * v_ptr
    else:
        t_act = t_ptr = rows["reward"].astype(np.float64)
        if alpha > 0:
            ap = np.asarray(act_prev, np.float64).reshape(n, 2)
            q = ap[np.arange(n), (rows["iaction"] != 0).astype(np.intp)]
            t_act = t_act + munchausen_term(q, soft_act(ap, tau_act), alpha, clip)
            t_ptr = t_ptr + munchausen_term(probe_prev, soft_prev, alpha, clip)
        live = np.where(rows["done"] != 0, 0.0, 1.0)
        y_act = t_act + float(gamma) * v_act * live
        y_ptr = t_ptr + float(gamma) * v_ptr * live
    pad = rows["ship"] < 0
    return np.where(pad, 0.0, y_act), np.where(pad, 0.0, y_ptr)


def target_bound(rows, alpha, clip, v, ret=None):
    """2e-6 * max(1, |reward| + |alpha * clip| + |V|) per row; in the n-step form the return stands where the reward
    does (y = ret + disc * V with disc <= 1: the same three roundings on the same magnitudes)."""
    r = rows["reward"].astype(np.float64) if ret is None else np.asarray(ret, np.float64)
    mag = np.abs(r) + abs(float(alpha) * float(clip)) + np.abs(np.asarray(v, np.float64))
    return TARGET_REL * np.maximum(1.0, mag)


# ---- the 9 hand-built observations of tests/test_gpu_soft_targets.py ----------------------------------------------
SIDE = 400
N_OBS = 9                            # the head kernel works on groups of 8 ships: one full group, one with a single ship


def _disc(plane, cy, cx, r):
    y, x = np.ogrid[:SIDE, :SIDE]
    plane |= (y - cy) ** 2 + (x - cx) ** 2 <= r * r


def observations():
    """(bits uint32 [9][2][5000], vec8 float32 [9][8]): a few ship discs (radius 10) and laser discs (radius 3) per
    observation, observation k with a ship disc that touches corner k % 4, packed on the host in the trunk's layout:
    pixel p = y * 400 + x is bit p & 31 of word p >> 5."""
    rs = np.random.RandomState(2021)
    maps = np.zeros((N_OBS, 2, SIDE, SIDE), bool)
    vec8 = np.zeros((N_OBS, 8), np.float32)
    e = SIDE - 1
    for k in range(N_OBS):
        ships = [(int(rs.randint(20, 380)), int(rs.randint(20, 380))) for _ in range(3 + k % 3)]
        ships.append([(4, 5), (3, e - 4), (e - 5, 2), (e - 3, e - 4)][k % 4])
        for cy, cx in ships:
            _disc(maps[k, 0], cy, cx, 10)
        for _ in range(4 + k % 4):
            _disc(maps[k, 1], int(rs.randint(0, SIDE)), int(rs.randint(0, SIDE)), 3)
        (y0, x0), (y1, x1) = ships[0], ships[1]
        vec8[k] = [float(k % 3) - 1.0, 1.0, x1, y1, SIDE, SIDE, x0, y0]
    words = np.zeros((N_OBS, 2, SIDE * SIDE // 32), np.uint32)
    flat = maps.reshape(N_OBS, 2, SIDE * SIDE)
    for bit in range(32):
        words |= flat[:, :, bit::32].astype(np.uint32) << np.uint32(bit)
    return words, vec8
