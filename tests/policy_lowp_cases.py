"""The cases of the 16-bit policy forward's tests (tests/test_policy_lowp_ref.py says how they were chosen): inputs from
the oracle's CPU rollout, the rounded graph's float64 reference and float32 yardstick per case, computed once and shared
by the CPU and the GPU test, and the bounds' bookkeeping.  A helper module (not collected)."""
import functools

import numpy as np
import torch

from tests import policy_lowp_ref as L
from tests.policy_fp64_cases import TOL_ACT, TOL_HEAT

SHARE_CAP = 0.02          # of a ship's 160 000 heat pixels beyond TOL_HEAT: a condition on the kernel, not a measurement
YARD_SHARE = SHARE_CAP / 4  # ... which the inputs have to leave room for: the fp32 yardstick stays at or below this
MODE = {1: "bf16", 2: "fp16"}
WEIGHT_SEED = 15
# the three cases of tests/test_gpu_policy_lowp.py: arenas (global ids), ships per arena, seed, ticks of [turret] * (M / 2) +
# [random] * (M - M / 2) (tests/policy_fp64_cases.rollout)
CASES = {"small": (tuple(range(4)), 4, 31, 40), "border": (tuple(range(4)), 4, 31, 40), "loop": ((0, 255, 256, 257, 299), 2, 19, 25)}
EDGE = (0, 1, 2, 7, 8, 199, 200, 391, 392, 398, 399, 400)   # test_trunk_sparse_is_bit_identical's border coordinates
BORDER_TICKS = 6                                             # all turrets, after the ships were placed


def border_xy(n, m):
    rs = np.random.RandomState(5)
    return rs.choice(EDGE, (n, m)), rs.choice(EDGE, (n, m))


@functools.lru_cache(maxsize=None)
def case_inputs(case):
    """(ship maps [n][400][400] u8, laser maps, heads [n][M][8] f64, weights) of a case, from the CPU oracle."""
    from oracle import pyoracle
    from ofighters_amd import _native as nat
    ids, M, seed, ticks = CASES[case]
    beh = np.array([nat.BEHAVIOURS[b] for b in ["turret"] * (M // 2) + ["random"] * (M - M // 2)], np.int32)
    arenas = []
    for g in ids:
        a = pyoracle.Arena(n_ships=M)
        a.spawn(pyoracle.reset_draws(a.cfg, seed, g, 0))
        for t in range(ticks):
            a.step(a.bot_actions(beh, seed, g, t))
        arenas.append(a)
    if case == "border":
        x, y = border_xy(len(ids), M)
        turrets = np.full(M, nat.BEHAVIOURS["turret"], np.int32)
        for k, (g, a) in enumerate(zip(ids, arenas)):
            pt = a.ships()["pt"]
            for i in range(M):
                a.set_ship(i, x[k, i], y[k, i], pt[i, 0], pt[i, 1])
            for t in range(ticks, ticks + BORDER_TICKS):
                a.step(a.bot_actions(turrets, seed, g, t))
    maps = [a.rasterise() for a in arenas]
    sm, lm = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    head = np.stack([a.obs_head()[0] for a in arenas])
    w, _ = pyoracle.policy_init(WEIGHT_SEED, trained_like=True)
    for v in (sm, lm, head, w):
        v.setflags(write=False)
    return sm, lm, head, w


def small_inputs():
    return case_inputs("small")


def rounded_pair(sm, lm, head, w, lowp, legacy, trunk_lowp):
    """Per arena the rounded graph in float64 (the reference) and in float32 (the yardstick): [(act, heat)], [(act, heat)]."""
    torch.set_num_threads(8)
    ref, yard = [], []
    for g in range(len(sm)):
        v = head[g].astype(np.float32)
        ref.append(L.forward(sm[g], lm[g], v, w, lowp, legacy_bilinear=legacy, trunk_lowp=trunk_lowp))
        yard.append(L.forward(sm[g], lm[g], v, w, lowp, dtype=torch.float32, legacy_bilinear=legacy, trunk_lowp=trunk_lowp))
    return ref, yard


def per_ship(got, ref):
    """L.stats of every ship of [(act [K][2], heat [K][400][400])] per arena against the reference of the same shape."""
    return [L.stats(ga[i], gh[i], ra[i], rh[i], TOL_HEAT) for (ga, gh), (ra, rh) in zip(got, ref) for i in range(len(ra))]


def summary(st):
    """The worst ship of a list of L.stats, figure by figure."""
    return {k: max(s[k] for s in st) for k in st[0] if k != "worst"}


def violations(st, act_tol=TOL_ACT, share_cap=SHARE_CAP):
    """The section's bounds: per ship act <= TOL_ACT and at most SHARE_CAP of the heat pixels beyond TOL_HEAT."""
    return [(i, s["act"], s["share"]) for i, s in enumerate(st) if not (s["act"] <= act_tol and s["share"] <= share_cap)]


@functools.lru_cache(maxsize=None)
def case_reference(case, lowp, legacy, trunk_lowp):
    """(reference, per-ship yardstick stats) of a case; computed once, shared by the tests, never written to."""
    sm, lm, head, w = case_inputs(case)
    ref, yard = rounded_pair(sm, lm, head, w, lowp, legacy, trunk_lowp)
    return ref, per_ship(yard, ref)


def small_reference(lowp, legacy, trunk_lowp):
    return case_reference("small", lowp, legacy, trunk_lowp)


def case_tag(case, lowp, legacy, trunk_lowp):
    return "%s_%s%s_%s" % (case, MODE[lowp], "_legacy_bilinear" if legacy else "", "stream" if trunk_lowp else "unfused")
