"""The pointer on the heat map's frame: k_head_stream<false, .> (the rollout's forward, no heat map stored) against
k_head_stream<true, .> (the forward that stores the heat map) and against the stored heat map itself.

The two instantiations run the same arithmetic, so the three pointers are EQUAL - no tolerance, no excluded case.  The
frame pixels are the ones that go through the zero-padding corrections of the consumers' pass (ofx_head.hip: column
lines walked a sub-step ahead, row lines from LDS), so the weights are built to put the maximum there:

  uprelu3 is positive on the whole plane (upconv3's BN beta is raised), and upconv4's kernel is
    'top'     tap row 0 strongly negative, tap row 1 positive, tap row 2 zero: pixels of heat-map row 0 lose the negative
              taps to the zero padding and are the only positive ones (the corners lose a positive tap too: smaller)
    'bottom', 'left', 'right': the same with tap row 2, tap column 0, tap column 2
    'corner'  centre tap + 4, the eight others - 1: a corner keeps 3 of them (positive), an edge 5, the interior 8

The test asserts FROM THE STORED HEAT MAP that the cases really land on the top and the bottom row, the left column
(left strip), the right column (right strip) and a corner - otherwise it would prove nothing.
"""
import numpy as np
import pytest

from tests.frame_cases import CASES, frame_weights, where

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("ships", [1, 8])
@pytest.mark.parametrize("legacy", [False, True])
def test_pointer_on_the_frame(legacy, ships):
    from ofighters_amd import ArenaBatch, _native as nat
    N, M, seed = 3, 8, 77
    b = ArenaBatch(N, M)
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    b.spawn_random(seed)
    for t in range(30):
        b.bot_actions(["turret"] * (M // 2) + ["random"] * (M - M // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    mask = np.zeros((N, M), np.uint8)
    if ships == 1:
        mask[:, 2] = 1   # the reference's line-up: one policy ship per arena
    else:
        mask[:] = 1
    seen = set()
    for ci, case in enumerate(CASES):
        w = frame_weights(case, 40 + ci)
        lean = b.policy_forward_host(w, ship_mask=mask)                  # k_head_stream<false, .>
        full = b.policy_forward_host(w, ship_mask=mask, want_heat=True)  # k_head_stream<true, .>
        for g in range(N):
            for i in range(M):
                if not mask[g, i]:
                    continue
                heat = full["heat"][g, i]
                k = int(np.argmax(heat))            # the first maximum in C order
                y, x = k // 400, k % 400
                lp, fp = tuple(int(v) for v in lean["ipointer"][g, i]), tuple(int(v) for v in full["ipointer"][g, i])
                print("legacy %d ships %d case %-6s arena %d ship %d: first maximum (y %3d, x %3d) = %.6g, lean pointer %s, "
                      "full pointer %s" % (legacy, ships, case, g, i, y, x, heat[y, x], lp, fp))
                assert fp == (x, y)
                assert lp == (x, y)
                assert np.array_equal(lean["act"][g, i], full["act"][g, i]) and lean["iaction"][g, i] == full["iaction"][g, i]
                seen.update(where(y, x))
                assert case in where(y, x), "the weights of case %r did not put the maximum there: (y %d, x %d)" % (case, y, x)
    b.close()
    assert seen >= set(CASES), seen
