"""OFX_OPT_POLICY_BF16 against a reference that rounds where the kernels round (tests/policy_lowp_ref.py, float64).

tests/test_gpu_policy_bf16.py can only hold the 16-bit forward to the UNROUNDED graph at 3e-2 / 4e-3, because the
legitimate operand rounding is itself 3e-3 / 3e-4: a defect smaller than the rounding passes it.  Against the rounded
graph the expected error is the fp32 path's own - TOL_ACT, TOL_HEAT of tests/test_gpu_policy_fp64.py - on all but the
few pixels behind an operand that sits on a 16-bit rounding boundary, which fp32 and float64 resolve differently.  Per
ship:
  act                          <= TOL_ACT
  heat pixels beyond TOL_HEAT  <= SHARE_CAP (2 %) of the 160 000 - a condition, not a measurement: the inputs are ones on
                               which an fp32 evaluation of the same rounded graph on the CPU (the yardstick,
                               tests/test_policy_lowp_ref.py) stays at a quarter of it; the three defects that test
                               plants put a third or more of the pixels out of bound
  heat max                     <= 4 x the yardstick's max over the same case (the convention of tests/test_gpu_fit_fp64.py),
                               never less than TOL_HEAT.  The tail IS boundary operands: which ones flip differs between
                               two fp32 evaluations, so a ship is held to the case's worst, not to its own yardstick
  ipointer                     the first maximum of the map the kernel wrote, and within 2 TOL_HEAT of the rounded float64
                               map's maximum
The cases: the small rollout in every form (mode x bilinear convention x streaming / unfused trunk - the unfused
trunk is fp32 with a 16-bit head: trunk_lowp=False), ships and lasers on the borders (halo columns, first / last row
tiles, strip edges), and 300 arenas (the persistent loop of k_trunk12 / k_conv3_stream and its double buffer).  Every
figure goes through _report of tests/test_gpu_policy_fp64.py into its report file under lowp_* tags, next to the yardstick's."""
import functools

import numpy as np
import pytest

from tests import policy_lowp_ref as L
from tests import policy_ref64 as R
from tests.policy_fp64_cases import TOL_ACT, TOL_HEAT, report as _report, rollout as _rollout
from tests.policy_lowp_cases import (BORDER_TICKS, CASES, SHARE_CAP, YARD_SHARE, border_xy, case_inputs, case_reference,
                                     case_tag, per_ship, summary, violations)

pytestmark = pytest.mark.gpu
# (tag, ship) -> allowed heat max, for a ship whose worst pixel was SHOWN to sit behind an operand within fp32 error of a
# rounding boundary (the report's "boundary" entry); empty: no ship needed it
WIDENED = {}


@functools.lru_cache(maxsize=None)
def _unrounded(case, legacy):
    """The declared graph in float64 (tests/policy_ref64.py): the distance to it is reported for context."""
    import torch
    torch.set_num_threads(8)
    sm, lm, head, w = case_inputs(case)
    return [R.forward(sm[g], lm[g], head[g].astype(np.float32), w, legacy_bilinear=legacy) for g in range(len(sm))]


def _same_inputs(b, case):
    """The device's maps and heads are the CPU rollout's the references were computed from."""
    from ofighters_amd import _native as nat
    sm, lm, head, _ = case_inputs(case)
    ids = list(CASES[case][0])
    gsm, glm = b.maps_host(nat.MAP_U8)
    ghead, _ = b.observe_head()
    assert np.array_equal(gsm[ids], sm) and np.array_equal(glm[ids], lm), case
    assert np.array_equal(ghead[ids], head), case


def _boundary(case, g, i, lowp, legacy, trunk_lowp, y, x):
    """For the report of a ship beyond the max bound: the smallest relative distance to a rounding boundary among the
    uprelu2 operands behind heat pixel (y, x) (5 x 5 x 4 around its low-res cell) and among the trunk's operands."""
    sm, lm, head, w = case_inputs(case)
    probe = {}
    L.forward(sm[g], lm[g], head[g].astype(np.float32), w, lowp, legacy_bilinear=legacy, trunk_lowp=trunk_lowp, _probe=probe)
    r, c = y // 4, x // 4
    win = probe["upconv3"][i, :, max(r - 2, 0):r + 3, max(c - 2, 0):c + 3]
    out = dict(uprelu2_window=float(L.boundary_distance(win, lowp).min()))
    for k in ("conv2", "conv3", "conv4"):
        if k in probe:
            out[k] = float(L.boundary_distance(probe[k], lowp).min())
    return out


def _check(case, got, pointers, lowp, legacy, trunk_lowp):
    """got: per arena (act [K][2], heat [K][400][400]); pointers: per arena [K][2]."""
    tag = "lowp_" + case_tag(case, lowp, legacy, trunk_lowp)
    ref, yst = case_reference(case, lowp, legacy, trunk_lowp)
    st = per_ship(got, ref)
    far = per_ship(got, _unrounded(case, legacy))
    ysum = summary(yst)
    assert not violations(yst, TOL_ACT / 4, YARD_SHARE), "the inputs leave the yardstick no room: change the inputs"
    max_tol = max(TOL_HEAT, 4 * ysum["max"])
    rec = dict(kernel=summary(st), yardstick=ysum, vs_unrounded=dict(act=summary(far)["act"], heat_max=summary(far)["max"]),
               heat_max_bound=max_tol, ships=len(st), per_ship=[dict(act=s["act"], share_interior=s["share_interior"],
                                                                      share_frame=s["share_frame"], max_interior=s["max_interior"],
                                                                      max_frame=s["max_frame"], yardstick_share=q["share"],
                                                                      yardstick_max=q["max"]) for s, q in zip(st, yst)])
    K = len(ref[0][0])
    over = [n for n, s in enumerate(st) if s["max"] > WIDENED.get((tag, n), max_tol)]
    if over:
        rec["boundary"] = {str(n): _boundary(case, n // K, n % K, lowp, legacy, trunk_lowp, *st[n]["worst"]) for n in over}
    _report(tag, rec)
    assert not violations(st), (tag, violations(st))
    assert not over, (tag, [(n, st[n]["max"], st[n]["worst"]) for n in over], max_tol, rec.get("boundary"))
    for g, ((_, heat), (_, h64), ptr) in enumerate(zip(got, ref, pointers)):
        for i in range(K):
            gx, gy = ptr[i]
            kk = int(np.argmax(heat[i]))
            assert (gx, gy) == (kk % 400, kk // 400), (tag, g, i)            # first maximum of the map the kernel wrote
            assert h64[i][gy, gx] >= h64[i].max() - 2 * TOL_HEAT * float(np.abs(h64[i]).max()), (tag, g, i)


def _forward(b, lowp, legacy, fuse):
    from ofighters_amd import _native as nat
    w = case_inputs("small")[3]
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    b.set_option(nat.OPT_TRUNK_FUSE, fuse)
    b.set_option(nat.OPT_POLICY_BF16, lowp)
    out = b.policy_forward_host(w, want_heat=True)
    return [(out["act"][g], out["heat"][g]) for g in range(b.N)], list(out["ipointer"])


@pytest.mark.parametrize("fuse", [1, 2])
@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("lowp", [1, 2])
def test_small_case_against_the_rounded_graph(lowp, legacy, fuse):
    """fuse = 2: the unfused trunk has no 16-bit form - an fp32 trunk under a 16-bit head stage B, what a small batch gets
    with OFX_OPT_TRUNK_FUSE on auto."""
    ids, M, seed, ticks = CASES["small"]
    b = _rollout(len(ids), M, seed=seed, ticks=ticks)
    _same_inputs(b, "small")
    got, ptr = _forward(b, lowp, legacy, fuse)
    b.close()
    _check("small", got, ptr, lowp, legacy, fuse == 1)


@pytest.mark.parametrize("lowp", [1, 2])
def test_border_case_against_the_rounded_graph(lowp):
    """Ships on x, y in {0, 1, 2, 7, 8, 199, 200, 391, 392, 398, 399, 400}, then turrets firing for a few ticks: non-constant
    operands in the halo columns, in the first and last row tiles of the 16-bit ts_gemm_phase and on the strip edges of
    tile_bf16."""
    ids, M, seed, ticks = CASES["border"]
    b = _rollout(len(ids), M, seed=seed, ticks=ticks)
    x, y = border_xy(len(ids), M)
    b.set_ships(x=x, y=y)
    for t in range(ticks, ticks + BORDER_TICKS):
        b.bot_actions(["turret"] * M, seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    _same_inputs(b, "border")
    got, ptr = _forward(b, lowp, False, 1)
    b.close()
    _check("border", got, ptr, lowp, False, True)


def test_persistent_loop_against_the_rounded_graph():
    """300 arenas: more images than workgroups, k_trunk12 and k_conv3_stream walk their img += gridDim.x loop.  Arenas
    0, 255, 256, 257, 299 are compared; the ship mask keeps the head (and the heat map) to them."""
    from ofighters_amd import DeviceBuffer, _native as nat
    ids, M, seed, ticks = CASES["loop"]
    N = 300
    b = _rollout(N, M, seed=seed, ticks=ticks)
    _same_inputs(b, "loop")
    w = case_inputs("loop")[3]
    S = N * M
    mask = np.zeros((N, M), np.uint8)
    mask[list(ids)] = 1
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    b.set_option(nat.OPT_POLICY_BF16, 1)
    dw, dm = DeviceBuffer(w.nbytes).upload(np.ascontiguousarray(w, np.float32)), DeviceBuffer(S).upload(mask)
    da, di, dp, dh = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S), DeviceBuffer(4 * S * 160000)
    b.policy_forward(dw.ptr, dm.ptr, da.ptr, di.ptr, dp.ptr, dh.ptr)
    b.sync()
    act, ptr = da.download(np.float32, (N, M, 2)), dp.download(np.int32, (N, M, 2))
    got = [(act[g], np.stack([dh.download(np.float32, (400, 400), offset=4 * (g * M + i) * 160000) for i in range(M)]))
           for g in ids]
    dh.free()
    b.close()
    _check("loop", got, [ptr[g] for g in ids], 1, False, True)
