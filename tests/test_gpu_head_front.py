"""The kernels between the trunk and k_head_stream - k_gemm_f32_splitk (dense1), k_head_dense, k_gemm_f32_k100 (updense1),
k_upconv1 and k_head_frames - at the smallest shapes where they can go wrong, against two yardsticks none of them is part of:

  FRAMES_REF  the forward with OFX_OPT_FRAMES_REF (k_head_frames_ref: the frame lines from the definition), with the bounds
              of tests/test_gpu_policy.py (TOL = 2e-5 of the tensor's maximum; act_values are bit-identical, the option only
              changes frame cells of the head)
  FLOAT64     the float64 graph of tests/policy_ref64.py, with the bounds of tests/test_gpu_policy_fp64.py

Shapes (arenas x ships): 1x1, 1x7, 1x8, 3x3, 17x1 - 1, 7, 8, 9 and 17 ships: the round-up of k_head_frames' grid to 8 and the
rotation of the ships inside a group of 8, M and N tiles of the GEMMs that are mostly outside the matrix.  Masks on 3x3: no
ship, a single ship, all but one.  One masked forward with 4100 selected ships, one per arena: k_upconv1's grid is bounded at
4096 workgroups, so the last four ships are second items of their workgroups.  Everything under both bilinear conventions.
Heat map, act_values, action and pointer are compared.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 2e-5                                          # tests/test_gpu_policy.py
TOL_ACT, TOL_HEAT, TOL_FRAME = 1.5e-5, 8e-6, 8e-6   # tests/test_gpu_policy_fp64.py
SHAPES = [(1, 1), (1, 7), (1, 8), (3, 3), (17, 1)]
F64_ARENAS = {(17, 1): (0, 8, 16)}                  # float64 on a sample there: the first ship of each group of 8


def _rollout(N, M, seed, ticks):
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, M)
    b.spawn_random(seed)
    for t in range(ticks):
        b.bot_actions(["turret"] * (M // 2) + ["random"] * (M - M // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    return b


def _weights():
    from oracle import pyoracle
    return pyoracle.policy_init(6, trained_like=True)[0]


def _both(b, w, legacy, mask=None):
    """The production forward and the FRAMES_REF forward of the same state."""
    from ofighters_amd import _native as nat
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    out = b.policy_forward_host(w, ship_mask=mask, want_heat=True)
    b.set_option(nat.OPT_FRAMES_REF, 1)
    ref = b.policy_forward_host(w, ship_mask=mask, want_heat=True)
    b.set_option(nat.OPT_FRAMES_REF, 0)
    return out, ref


def _f64(b, w, legacy, arenas):
    """{arena: (act64 [M][2], heat64 [M][400][400])}"""
    import torch
    from ofighters_amd import _native as nat
    from tests import policy_ref64 as R
    torch.set_num_threads(8)
    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_U8)
    return {g: R.forward(sm[g], lm[g], head[g].astype(np.float32), w, legacy_bilinear=legacy) for g in arenas}


@functools.lru_cache(maxsize=None)
def _case(N, M, legacy):
    """One rollout per (shape, convention): computed once, shared by the tests below, never modified."""
    b = _rollout(N, M, seed=8 + N + M, ticks=30)
    w = _weights()
    out, ref = _both(b, w, legacy)
    f64 = _f64(b, w, legacy, F64_ARENAS.get((N, M), range(N)))
    b.close()
    return out, ref, f64


def check_frames_ref(out, ref, ships):
    hs = float(np.abs(ref["heat"]).max())
    for g, i in ships:
        np.testing.assert_allclose(out["heat"][g, i], ref["heat"][g, i], rtol=0, atol=TOL * hs)
        assert np.array_equal(out["act"][g, i], ref["act"][g, i])
        assert out["iaction"][g, i] == ref["iaction"][g, i]
        gx, gy = out["ipointer"][g, i]
        k = int(np.argmax(out["heat"][g, i]))       # the pointer is the first maximum of the map the kernel wrote
        assert (gx, gy) == (k % 400, k // 400)
        assert ref["heat"][g, i][gy, gx] >= ref["heat"][g, i].max() - 2 * TOL * hs


def check_f64(out, f64, ships):
    from tests import policy_ref64 as R
    worst = np.zeros(3)
    for g, i in ships:
        a64, h64 = f64[g][0][i], f64[g][1][i]
        worst = np.maximum(worst, R.errors(out["act"][g, i], out["heat"][g, i], a64, h64))
        gx, gy = out["ipointer"][g, i]
        assert h64[gy, gx] >= h64.max() - 2 * TOL_HEAT * float(np.abs(h64).max())
        if abs(float(a64[0] - a64[1])) > 2 * TOL_ACT * max(1.0, float(np.abs(a64).max())):
            assert out["iaction"][g, i] == int(np.argmax(a64))
    print("max |err| / max |value| against float64: act %.3g, heat interior %.3g, heat frame %.3g" % tuple(worst))
    assert worst[0] <= TOL_ACT and worst[1] <= TOL_HEAT and worst[2] <= TOL_FRAME, worst


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_frames_ref(shape, legacy):
    N, M = shape
    out, ref, _ = _case(N, M, legacy)
    check_frames_ref(out, ref, [(g, i) for g in range(N) for i in range(M)])


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_float64(shape, legacy):
    N, M = shape
    out, _, f64 = _case(N, M, legacy)
    check_f64(out, f64, [(g, i) for g in sorted(f64) for i in range(M)])


@pytest.mark.parametrize("legacy", [False, True])
def test_ship_masks(legacy):
    """No ship, a single ship, all but one: the selected ships against both yardsticks and equal to their values in the
    unmasked forward (a ship's result does not depend on its place in the list); the forward behind an empty mask is
    the unmasked one again."""
    N, M = 3, 3
    b = _rollout(N, M, seed=8 + N + M, ticks=30)
    w = _weights()
    full, _ = _both(b, w, legacy)
    f64 = _f64(b, w, legacy, range(N))
    none = np.zeros((N, M), np.uint8)
    single = none.copy()
    single[1, 1] = 1
    but_one = np.ones((N, M), np.uint8)
    but_one[2, 0] = 0
    _both(b, w, legacy, mask=none)                   # nothing to compare: it must run, and leave the next forwards alone
    for mask in (single, but_one):
        out, ref = _both(b, w, legacy, mask=mask)
        ships = [(g, i) for g in range(N) for i in range(M) if mask[g, i]]
        check_frames_ref(out, ref, ships)
        check_f64(out, f64, ships)
        for g, i in ships:
            for k in full:
                assert np.array_equal(out[k][g, i], full[k][g, i]), (k, g, i)
    again, _ = _both(b, w, legacy)
    for k in full:
        assert np.array_equal(again[k], full[k]), k
    b.close()


@pytest.mark.parametrize("legacy", [False, True])
def test_more_selected_ships_than_upconv1_workgroups(legacy):
    """4100 arenas x 2 ships, ship 1 of every arena selected: 4100 items on k_upconv1's 4096 workgroups.  act_values,
    action and pointer of every selected ship against FRAMES_REF; the heat map of the ships around the wrap (items 0,
    4095, 4096, 4099) against FRAMES_REF, of the two behind it against float64."""
    from ofighters_amd import DeviceBuffer, _native as nat
    N, M = 4100, 2
    S = N * M
    b = _rollout(N, M, seed=21, ticks=12)
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    w = _weights()
    mask = np.zeros((N, M), np.uint8)
    mask[:, 1] = 1
    sample = (0, 4095, 4096, 4099)
    dw, dm = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(S).upload(mask)
    da, di, dp, dh = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S), DeviceBuffer(4 * S * 160000)
    res = []
    for frames_ref in (0, 1):
        b.set_option(nat.OPT_FRAMES_REF, frames_ref)
        b.policy_forward(dw.ptr, dm.ptr, da.ptr, di.ptr, dp.ptr, dh.ptr)
        b.sync()
        # only the sampled maps are downloaded
        heat = {g: dh.download(np.float32, (400, 400), offset=4 * (g * M + 1) * 160000) for g in sample}
        res.append(dict(act=da.download(np.float32, (N, M, 2)), iaction=di.download(np.int32, (N, M)),
                        ipointer=dp.download(np.int32, (N, M, 2)), heat=heat))
    b.set_option(nat.OPT_FRAMES_REF, 0)
    out, ref = res
    assert np.array_equal(out["act"][:, 1], ref["act"][:, 1]) and np.array_equal(out["iaction"][:, 1], ref["iaction"][:, 1])
    # the pointers of the two forwards may differ only where the frame lines' rounding moves a tie: checked on the maps below
    hs = max(float(np.abs(ref["heat"][g]).max()) for g in sample)
    for g in sample:
        np.testing.assert_allclose(out["heat"][g], ref["heat"][g], rtol=0, atol=TOL * hs)
        gx, gy = out["ipointer"][g, 1]
        k = int(np.argmax(out["heat"][g]))
        assert (gx, gy) == (k % 400, k // 400)
        assert ref["heat"][g][gy, gx] >= ref["heat"][g].max() - 2 * TOL * hs
    f64 = _f64(b, w, legacy, (4096, 4099))
    flat = dict(act=out["act"], iaction=out["iaction"], ipointer=out["ipointer"],
                heat={(g, 1): out["heat"][g] for g in sample})   # heat[g, i], as check_f64 indexes it
    check_f64(flat, f64, [(4096, 1), (4099, 1)])
    for d in (dw, dm, da, di, dp, dh):
        d.free()
    b.close()

