"""tests/policy_lowp_ref.py - the graph with the 16-bit forward's operand rounding - checked WITHOUT a GPU: that it is the
declared graph when nothing is rounded (the phase-form algebra and the frame handling), that its rounding is to nearest
even, what an fp32 evaluation of the same rounded graph loses against the float64 one on the inputs of the GPU test's
small case (the YARDSTICK: the bounds of tests/test_gpu_policy_lowp.py have to hold for it with a factor 4 to spare),
and that three defects the comparison with the unrounded graph cannot see break those bounds.

The inputs are the states of the GPU test's three cases (the small one is the rollout of tests/test_gpu_policy_bf16.py:
4 arenas x 4 ships, seed 31, 40 ticks, two turrets and two random bots per arena) rebuilt from the oracle's CPU rollout,
which is bit-exact against the device's (tests/test_gpu_step.py); the GPU test asserts that its maps and heads ARE these.

The yardstick is evaluated in a written-down order of elementwise float32 operations (policy_lowp_ref.conv_fixed,
dense_fixed, upsample2_fixed), not through the libraries' convolutions and matrix products: those give other bits with
another thread count or instruction set (the same inputs gave 0.22 % and 0.29 % of a ship's pixels on two machines),
and a bound derived from a figure that moves is a test that flickers.

The weights are policy_init(15, trained_like=True), not the policy_init(5, ..) of test_gpu_policy_bf16.py.  How many
pixels an fp32 evaluation moves beyond TOL_HEAT depends on the weights (the error is normalised by the map's maximum,
and every flipped operand moves the ~200 pixels behind it): with seed 5 the yardstick reaches 0.61 % of a ship's
pixels on the real rollout, above the 0.5 % the cap of 2 % is conditioned on.  Over the small case's 8 forms, the border
case and the loop case the yardstick's worst ship had, for the seeds 5 .. 16: 0.61, 0.36, 0.73, -, 3.6, 0.81, 0.99, 0.59, 0.57,
0.84, 0.49, 0.95 % (seed 8 not rerun: 2 % through the libraries).  Seed 6 stays below 0.5 % because its heat map barely
depends on the trunk - and for the same reason conv4's operands left unrounded in fp16 move NO ship out of bound
with it.  Seed 15 is the one that leaves the yardstick its room AND shows every planted defect on every ship.  The
choice was made on these CPU figures alone, before any kernel was compared."""
import numpy as np
import pytest
import torch

from tests import policy_lowp_ref as L
from tests import policy_ref64 as R
from tests.policy_fp64_cases import TOL_ACT, TOL_HEAT, report as _report
from tests.policy_lowp_cases import (CASES, MODE, YARD_SHARE, case_reference, case_tag, per_ship, small_inputs,
                                     small_reference, summary, violations)


@pytest.mark.parametrize("legacy", [False, True])
def test_unrounded_is_the_declared_graph(legacy):
    """lowp = 0: only the float32 BatchNorm fold separates the phase form + frame lines from policy_ref64.forward
    (measured 5e-8 of the heat map's maximum; the fold's own rounding is 2^-24 = 6e-8 per factor)."""
    sm, lm, head, w = small_inputs()
    torch.set_num_threads(8)
    for g in (0, 3):
        v = head[g].astype(np.float32)
        a64, h64 = R.forward(sm[g], lm[g], v, w, legacy_bilinear=legacy)
        a, h = L.forward(sm[g], lm[g], v, w, 0, legacy_bilinear=legacy)
        af, hf = L.forward(sm[g], lm[g], v, w, 0, legacy_bilinear=legacy, fixed_order=True)   # the yardstick's own operations
        for i in range(4):
            err = R.errors(a[i], h[i], a64[i], h64[i])
            print("unrounded vs declared, arena %d ship %d legacy %d: act %.2e interior %.2e frame %.2e" % ((g, i, legacy) + err))
            assert max(err) <= 5e-7, (g, i, err)
            assert max(R.errors(af[i], hf[i], a64[i], h64[i])) <= 5e-7, (g, i)


def _rne_bits(x, lowp):
    """float32 -> bf16 / fp16 -> float32 by explicit bit manipulation, round to nearest even (python ints, one value)."""
    u = int(np.float32(x).view(np.uint32))
    sign, e, m = u >> 31, (u >> 23) & 0xFF, u & 0x7FFFFF
    assert e != 0 and e != 0xFF              # the vector holds normal float32 values (and zero, handled by the caller)
    if lowp == 1:                            # bf16: the top 16 bits, ties to the even one
        r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return float(np.uint32(r).view(np.float32))
    mant = m | 0x800000                      # |x| = mant * 2^(e - 150)
    drop = 13 if e >= 113 else 13 + (113 - e)  # fp16 normal: 10 fraction bits; below 2^-14: the quantum stays 2^-24
    if drop > 25:
        q = 0
    else:
        q, rem, half = mant >> drop, mant & ((1 << drop) - 1), 1 << (drop - 1)
        q += rem > half or (rem == half and (q & 1))
    val = q * 2.0 ** (e - 150 + drop)
    if val >= 65520.0:                       # past the largest finite fp16 + half a quantum: overflow
        val = float("inf")
    return -val if sign else val


@pytest.mark.parametrize("lowp", [1, 2])
def test_rounding_helper_is_nearest_even(lowp):
    f = np.float32
    core = []
    q = {1: 2.0 ** -7, 2: 2.0 ** -10}[lowp]               # the quantum of the format in [1, 2)
    for base in (1.0, 1.0 + q, 1.0 + 2 * q, 1.5, 2.0 - 2 * q, 2.0 - q, 0.3, 3.0e-3, 37.0):
        s = 2.0 ** np.floor(np.log2(base))
        tie = f(base + 0.5 * q * s)                          # exactly between two neighbours (base is representable up to s)
        core += [f(base), tie, np.nextafter(tie, f(0)), np.nextafter(tie, f(1e9))]
    for p2 in (0.5, 1.0, 2.0, 2.0 ** -14, 2.0 ** -24, 2.0 ** -25):
        core += [f(p2), np.nextafter(f(p2), f(0)), np.nextafter(f(p2), f(1e9)), f(p2 * (1 - q / 4)), f(p2 * (1 - q / 2))]
    # fp16 subnormals (quantum 2^-24): ties at odd multiples of 2^-25, both neighbours; the smallest normal from below
    for k in (1, 3, 5, 1023 * 2 + 1, 2047):
        tie = f(k * 2.0 ** -25)
        core += [tie, np.nextafter(tie, f(0)), np.nextafter(tie, f(1)), f((k // 2 + 1) * 2.0 ** -24)]
    core += [f(65504.0), np.nextafter(f(65504.0), f(0)), np.nextafter(f(65504.0), f(1e9)), f(65519.996), f(65520.0),
             np.nextafter(f(65520.0), f(0)), np.nextafter(f(65520.0), f(1e9)), f(65536.0)]
    x = np.array(core + [-c for c in core], np.float32)
    want = np.array([_rne_bits(c, lowp) for c in x], np.float64)
    assert len(np.unique(x)) > 120
    for dtype in (torch.float32, torch.float64):
        got = L.round_lowp(torch.from_numpy(x).to(dtype), lowp)
        assert got.dtype == dtype
        assert np.array_equal(got.to(torch.float64).numpy(), want), x[got.to(torch.float64).numpy() != want]
    assert np.array_equal(L.round_lowp(torch.zeros(2), lowp).numpy(), np.zeros(2, np.float32))
    # the vector does hold ties that go both ways, and values the truncation of the mutant treats differently
    ties = want[1:4 * 9:4] if lowp == 1 else None
    if lowp == 1:
        assert (ties < x[1:4 * 9:4]).any() and (ties > x[1:4 * 9:4]).any()
        assert not np.array_equal(L.truncate_bf16(torch.from_numpy(x)).numpy().astype(np.float64), want)
    else:
        assert np.isinf(want).sum() == 6 and (want[np.abs(x) < 2.0 ** -14] != 0).any() and (want[x != 0] == 0).any()


# every form the GPU test compares: (case, lowp, legacy, trunk_lowp)
FORMS = ([("small", l, g, t) for l in (1, 2) for g in (False, True) for t in (True, False)]
         + [("border", 1, False, True), ("border", 2, False, True), ("loop", 1, False, True)])


@pytest.mark.parametrize("case,lowp,legacy,trunk_lowp", FORMS)
def test_yardstick_leaves_room_under_the_bounds(case, lowp, legacy, trunk_lowp):
    """The rounded graph in float32 against itself in float64, per ship: act and the share of heat pixels beyond TOL_HEAT
    stay at a quarter of what the GPU test allows the kernel; the heat map's max is REPORTED (operands on a rounding
    boundary: it has no bound of its own, the GPU test allows the kernel 4x this figure)."""
    _, st = case_reference(case, lowp, legacy, trunk_lowp)
    assert len(st) == len(CASES[case][0]) * CASES[case][1]
    _report("lowp_yardstick_" + case_tag(case, lowp, legacy, trunk_lowp), dict(summary(st), ships=len(st), tol_heat=TOL_HEAT))
    assert not violations(st, TOL_ACT / 4, YARD_SHARE), violations(st, TOL_ACT / 4, YARD_SHARE)


@pytest.mark.parametrize("legacy", [False, True])
@pytest.mark.parametrize("mutant,lowp", [("conv3_truncate", 1), ("conv4_unrounded", 1), ("conv4_unrounded", 2),
                                         ("upconv3_round_before_phase", 1), ("upconv3_round_before_phase", 2)])
def test_mutants_break_the_bounds(mutant, lowp, legacy):
    """Each defect, evaluated in float64 so that nothing but the defect separates it from the reference, puts EVERY ship
    outside the bounds the GPU test asserts (share of pixels, or act) - and stays inside those of test_gpu_policy_bf16.py."""
    sm, lm, head, w = small_inputs()
    ref, _ = small_reference(lowp, legacy, True)
    torch.set_num_threads(8)
    got = [L.forward(sm[g], lm[g], head[g].astype(np.float32), w, lowp, legacy_bilinear=legacy, _mutate=mutant)
           for g in range(4)]
    st = per_ship(got, ref)
    bad = violations(st)
    _report("lowp_mutant_%s_%s%s" % (mutant, MODE[lowp], "_legacy_bilinear" if legacy else ""),
            dict(summary(st), ships_out_of_bound=len(bad), ships=len(st), min_share=min(s["share"] for s in st)))
    assert len(bad) == len(st), (mutant, len(bad))
    assert summary(st)["max"] <= {1: 3e-2, 2: 4e-3}[lowp]          # the looser comparison lets it through
