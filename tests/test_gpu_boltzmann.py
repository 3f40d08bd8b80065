"""Boltzmann exploration on the device: ofx_policy_act_boltzmann against the float64 reference of
tests/boltzmann_oracle.py (the noise, the temperatures, both heads' choice, the acceptance rule for near-ties), against
ofx_policy_act where the two must agree bit for bit (temperature 0, the collecting phase), on the geometry of the head
kernel (frame rows and columns, a corner, the seam between a ship's two workgroups), and through TrainingRollout with a
checkpoint in the middle.

3 arenas x 2 ships under the mask [[1, 0], [0, 1], [1, 1]] (the compacted list index of a ship differs from its ship
index), on a handle whose first global arena is 5 (the noise is keyed by the GLOBAL arena)."""
import math

import numpy as np
import pytest

from tests import boltzmann_oracle as bo

pytestmark = pytest.mark.gpu

W = H = 400
N, M, BASE = 3, 2, 5
S = N * M
SEED = 0x0F160B17
MASK = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
SEL = [(a, i) for a in range(N) for i in range(M) if MASK[a, i]]
SENTINEL = np.float32(-12345.0)


class _Rig:
    """A handle with the weights, the mask and the buffers of one test."""

    def __init__(self, arena_base=BASE):
        from ofighters_amd import ArenaBatch, DeviceBuffer
        from ofighters_amd.agents.policy_weights import synthetic
        self.b = ArenaBatch(N, M, arena_base=arena_base)
        self.b.spawn_random(SEED)
        w = synthetic(7)
        self.w = DeviceBuffer(w.nbytes).upload(w)
        self.m = DeviceBuffer(MASK.nbytes).upload(MASK)
        self.vals = [DeviceBuffer(4 * S) for _ in range(4)]
        self.act_d, self.ia_d, self.ip_d = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S)
        self.heat_d = DeviceBuffer(4 * S * W * H)

    def sentinels(self):
        self.b.sync()
        for v in self.vals:
            v.upload(np.full(S, SENTINEL, np.float32))

    def ptrs(self):
        return dict(q_sa_ptr=self.vals[0].ptr, p_sp_ptr=self.vals[1].ptr, v_act_ptr=self.vals[2].ptr, v_ptr_ptr=self.vals[3].ptr)

    def values(self):
        self.b.sync()
        return [v.download(np.float32, (N, M)) for v in self.vals]

    def forward(self):
        """(act [N][M][2], heat [N][M][H][W], greedy pointer [N][M][2]) of the current state, into the test's buffers
        (the handle's kept results stay)."""
        self.b.policy_forward(self.w.ptr, self.m.ptr, self.act_d.ptr, self.ia_d.ptr, self.ip_d.ptr, self.heat_d.ptr)
        self.b.sync()
        return (self.act_d.download(np.float32, (N, M, 2)), self.heat_d.download(np.float32, (N, M, H, W)),
                self.ip_d.download(np.int32, (N, M, 2)))

    def chosen(self):
        """The handle's kept (iaction, ipointer) as the packed actions show them."""
        self.b.policy_actions(ship_mask_ptr=self.m.ptr)
        return self.b.actions_host()

    def advance(self, tick):
        self.b.bot_actions(["random"] * M, SEED, tick=tick)
        self.b.policy_actions(ship_mask_ptr=self.m.ptr)
        self.b.step()

    def close(self):
        self.b.close()


# ------------------------------------------------------------------------------ 1. the float32 Gumbel function
def test_gumbel_against_float64():
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(1, 2)
    words = np.concatenate([bo.edge_words(), bo.philox_words(SEED, 0, np.arange(1 << 18), 0, 6).reshape(-1)])
    assert len(words) >= (1 << 20) + 90
    g = b.policy_gumbel(words)
    b.close()
    assert g.dtype == np.float32 and np.isfinite(g).all()
    err = float(np.abs(g.astype(np.float64) - bo.gumbel(words)).max())
    print("largest |g - float64| = %.3e (GUMBEL_ABS_ERR %.3e)" % (err, bo.GUMBEL_ABS_ERR))
    assert err <= bo.GUMBEL_ABS_ERR and err <= 1e-4


# ------------------------------------------------------------------------------ 2. / 3. where it must be ofx_policy_act
@pytest.mark.parametrize("collecting", [0, 1], ids=["temperature0", "collecting"])
def test_equals_policy_act_bit_for_bit(collecting):
    """tau = (0, 0) is ofx_policy_act(epsilon = 0); collecting != 0 is ofx_policy_act(collecting = 1) whatever tau is."""
    a, b = _Rig(), _Rig()
    tau = (0.7, 0.3) if collecting else (0.0, 0.0)
    for tick in range(5):
        a.sentinels(), b.sentinels()
        a.b.policy_act_boltzmann(a.w.ptr, 0.5, tau[0], tau[1], SEED, tick=tick, collecting=collecting, ship_mask_ptr=a.m.ptr,
                                 **a.ptrs())
        b.b.policy_act(b.w.ptr, 0.5 if collecting else 0.0, SEED, tick=tick, collecting=collecting, ship_mask_ptr=b.m.ptr,
                       **b.ptrs())
        got, want = a.chosen(), b.chosen()
        assert got[MASK != 0].tobytes() == want[MASK != 0].tobytes(), tick     # (policy_actions writes the selected ships only)
        for g, w_ in zip(a.values(), b.values()):
            assert g.tobytes() == w_.tobytes(), tick
            assert (g[MASK == 0] == SENTINEL).all() and (g[MASK != 0] != SENTINEL).all()
        a.advance(tick), b.advance(tick)
    a.close(), b.close()


# ------------------------------------------------------------------------------ 4. sampling at moderate temperature
EPSILON = 0.8
LADDER = [1.0, 2.5, float("inf")]


def _check_sampled(rig, tick, tau, expo, stats):
    """One ofx_policy_act_boltzmann call against the oracle, on the heat maps of the same state and options."""
    act, heat, greedy = rig.forward()
    rig.sentinels()
    rig.b.policy_act_boltzmann(rig.w.ptr, EPSILON, tau[0], tau[1], SEED, tick=tick, ship_mask_ptr=rig.m.ptr, **rig.ptrs())
    got = rig.chosen()
    q_sa, p_sp, v_act, v_ptr = rig.values()
    T_act, T_ptr = bo.temperatures(tau[0], EPSILON, expo, N), bo.temperatures(tau[1], EPSILON, expo, N)
    for (a, i) in SEL:
        ia, px, py = int(got["thrust"][a, i]), int(got["px"][a, i]), int(got["py"][a, i])
        assert got["shoot"][a, i] == 1 - ia and 0 <= px < W and 0 <= py < H
        g = bo.noise_map(SEED, BASE + a, i, tick) if T_ptr[a] != 0 else None
        ref = bo.perturbed(heat[a, i], T_ptr[a], g)
        assert bo.accepted(ref, py * W + px, T_ptr[a]), (tick, a, i, px, py, float(ref[py, px]), float(ref.max()))
        exact = int(np.argmax(ref))
        stats["pointer_differs"] += exact != py * W + px
        top = np.partition(ref.reshape(-1), -2)[-2:]
        stats["gaps"].append(float(top[1] - top[0]) / max(float(T_ptr[a]), 1e-30) if T_ptr[a] != 0 else math.inf)
        stats["moved"] += T_ptr[a] != 0 and (px, py) != tuple(greedy[a, i])
        if T_ptr[a] == 0:
            assert (px, py) == tuple(greedy[a, i])                     # a greedy arena: the arg-max itself
        g01 = bo.action_noise(SEED, BASE + a, i, tick) if T_act[a] != 0 else None
        pa = bo.perturbed(act[a, i], T_act[a], g01)
        assert bo.accepted(pa, ia, T_act[a]), (tick, a, i, ia, pa)
        stats["action_differs"] += bo.choose_action(act[a, i], T_act[a], g01) != ia
        stats["action_moved"] += ia != int(act[a, i, 1] > act[a, i, 0])
        # the four values: raw, bit for bit
        assert p_sp[a, i] == heat[a, i, py, px], (tick, a, i)
        assert v_ptr[a, i] == heat[a, i].max()
        assert q_sa[a, i] == act[a, i, ia] and v_act[a, i] == act[a, i].max()
    for v in (q_sa, p_sp, v_act, v_ptr):
        assert (v[MASK == 0] == SENTINEL).all()                        # unselected ships are not written
    stats["cases"] += len(SEL)


def test_sampled_choices_are_the_oracles():
    from ofighters_amd import _native as nat
    rig = _Rig()
    act, heat, _ = rig.forward()
    h0 = heat[SEL[0]]
    tau = (float(abs(act[SEL[0]][1] - act[SEL[0]][0])), 0.25 * float(h0.max() - np.median(h0)))
    assert tau[0] > 0 and tau[1] > 0
    stats = dict(pointer_differs=0, action_differs=0, moved=0, action_moved=0, cases=0, gaps=[])
    for tick in range(6):
        rig.b.policy_epsilon_ladder(None)
        _check_sampled(rig, tick, tau, None, stats)
        rig.b.policy_epsilon_ladder(np.array(LADDER))
        _check_sampled(rig, tick, tau, LADDER, stats)
        rig.advance(tick)
    rig.b.policy_epsilon_ladder(None)
    rig.b.set_option(nat.OPT_POLICY_BF16, 1)                           # once more on the 16-bit forward's own heat map
    _check_sampled(rig, 6, tau, None, stats)
    rig.close()
    finite = [g for g in stats["gaps"] if math.isfinite(g)]
    print("tau %r; %d cases: pointer differs from the exact arg-max in %d, action in %d; %d pointers and %d actions moved off "
          "the greedy choice; smallest gap between the two largest perturbed values %.3e T (median %.3e T)"
          % (tau, stats["cases"], stats["pointer_differs"], stats["action_differs"], stats["moved"], stats["action_moved"],
             min(finite), float(np.median(finite))))
    assert stats["cases"] == 13 * len(SEL)
    assert stats["pointer_differs"] + stats["action_differs"] <= 1
    assert stats["moved"] >= 10 and stats["action_moved"] >= 1         # the temperature did something


# ------------------------------------------------------------------------------ 5. geometry: the noise alone decides
# (name, tick, x, y) for ship 0 of local arena 0 (global arena 5): ticks whose largest noise value lies on the frame of
# the map, on a corner, and on either side of the seam between the two workgroups of a ship (x = 199 | 200); found by
# a search over the oracle's noise alone, with the two largest values at least 0.3 apart
GEOMETRY = [("row 0", 96, 37, 0), ("row 399", 220, 5, 399), ("column 0", 2050, 0, 299), ("column 399", 70, 399, 386),
            ("seam, left", 270, 199, 202), ("seam, right", 844, 200, 150), ("corner", 4670, 0, 399)]


def test_geometry_under_noise_alone():
    rig = _Rig()
    _, heat, _ = rig.forward()
    T = np.float32(1e30)
    for name, tick, x, y in GEOMETRY:
        g = bo.noise_map(SEED, BASE, 0, tick)
        k = int(np.argmax(g))
        top = np.partition(g.reshape(-1), -2)[-2:]
        assert (k % W, k // W) == (x, y) and top[1] - top[0] >= 0.3, name        # the oracle still says so
        assert bo.choose_pointer(heat[0, 0], T, g) == (x, y), name
        rig.sentinels()
        rig.b.policy_act_boltzmann(rig.w.ptr, 1.0, 0.0, 1e30, SEED, tick=tick, ship_mask_ptr=rig.m.ptr, **rig.ptrs())
        got = rig.chosen()
        assert (int(got["px"][0, 0]), int(got["py"][0, 0])) == (x, y), name
        q_sa, p_sp, v_act, v_ptr = rig.values()
        assert p_sp[0, 0] == heat[0, 0, y, x] and v_ptr[0, 0] == heat[0, 0].max(), name
        for (a, i) in SEL[1:]:                                                  # and the other ships, any pixel
            ga = bo.noise_map(SEED, BASE + a, i, tick)
            assert bo.choose_pointer(heat[a, i], T, ga) == (int(got["px"][a, i]), int(got["py"][a, i])), (name, a, i)
    assert {x for _, _, x, _ in GEOMETRY} >= {0, 199, 200, 399} and {y for _, _, _, y in GEOMETRY} >= {0, 399}
    rig.close()


def test_argument_checks():
    from ofighters_amd import OfxError, _native as nat
    rig = _Rig()
    rig.b.policy_act(rig.w.ptr, 0.3, SEED, tick=0)                    # the handle's values: kept, and must stay
    rig.b.sync()
    for tau in ((-1.0, 1.0), (1.0, -1e-9), (float("nan"), 1.0), (1.0, float("inf"))):
        for collecting in (0, 1):
            with pytest.raises(OfxError) as err:
                rig.b.policy_act_boltzmann(rig.w.ptr, 0.5, tau[0], tau[1], SEED, tick=0, collecting=collecting)
            assert err.value.code == nat.OFX_ERR_INVALID
    with pytest.raises(OfxError) as err:
        rig.b.policy_act_boltzmann(rig.w.ptr, 1.5, 1.0, 1.0, SEED, tick=0)
    assert err.value.code == nat.OFX_ERR_INVALID
    rig.close()


# ------------------------------------------------------------------------------ 6. the rollout, with a checkpoint
N6, M6, STEPS6, TAU6 = 4, 2, 8, (0.05, 0.02)


def _build6():
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N6, M6, arena_base=BASE)
    eps = Epsilon_decay()
    eps.set(0.9)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=8,
                       prioritized=True, actor_priorities=True)
    roll = TrainingRollout(b, tr, ["random"] * M6, SEED, policy_ships=(0, 1), episode_ticks=20, collecting_steps=2,
                           replay_every=3, replay_on_death=False, eval_arenas=1, total_arenas=BASE + N6, boltzmann=TAU6)
    return b, tr, roll


def _state6(b, tr):
    b.sync()
    return dict(weights=tr.weights_host().tobytes(), rows=[b.replay_rows(g).tobytes() for g in range(b.N)],
                mass=[b.replay_priorities(g).tobytes() for g in range(b.N)], fit_steps=tr.fit_steps)


def test_rollout_samples_and_resumes(tmp_path):
    from ofighters_amd import DeviceBuffer
    b, tr, roll = _build6()
    expo = b.policy_epsilon_ladder_host()
    assert np.isinf(expo[-1]) and (expo[:-1] == 1.0).all()
    Sn = N6 * M6
    act_d, ia_d, ip_d, heat_d = DeviceBuffer(8 * Sn), DeviceBuffer(4 * Sn), DeviceBuffer(8 * Sn), DeviceBuffer(4 * Sn * W * H)
    played, moved = [], 0
    path = str(tmp_path / "ck")
    for t in range(STEPS6):
        if t == 4:
            mid = _state6(b, tr)
            roll.checkpoint(path)
        collecting = t + 1 < roll.collecting_steps
        eps = tr.epsilon.get()
        # the forward of the state the decision is taken on, into buffers of the test
        b.policy_forward(tr.weights.ptr, roll._mask.ptr, act_d.ptr, ia_d.ptr, ip_d.ptr, heat_d.ptr)
        b.sync()
        act, heat = act_d.download(np.float32, (N6, M6, 2)), heat_d.download(np.float32, (N6, M6, H, W))
        greedy = ip_d.download(np.int32, (N6, M6, 2))
        roll.lockstep()
        got = b.actions_host()
        played.append(got.copy())
        assert roll.capture_tick == t + 1
        for a in range(N6):
            for i in range(M6):
                ia, px, py = int(got["thrust"][a, i]), int(got["px"][a, i]), int(got["py"][a, i])
                if a == N6 - 1:                                    # the evaluation arena: greedy, the collecting phase too
                    assert (px, py) == tuple(greedy[a, i]) and ia == int(act[a, i, 1] > act[a, i, 0]), (t, i)
                elif not collecting:
                    Ta, Tp = bo.temperatures(TAU6[0], eps, n=1)[0], bo.temperatures(TAU6[1], eps, n=1)[0]
                    ref = bo.perturbed(heat[a, i], Tp, bo.noise_map(SEED, BASE + a, i, t))
                    assert bo.accepted(ref, py * W + px, Tp), (t, a, i)
                    assert bo.accepted(bo.perturbed(act[a, i], Ta, bo.action_noise(SEED, BASE + a, i, t)), ia, Ta), (t, a, i)
                    moved += (px, py) != tuple(greedy[a, i])
    assert moved >= 4
    end = _state6(b, tr)
    assert tr.fit_steps >= 2 and end["weights"] != mid["weights"]
    # the rows carry the sampled choices: the row that starts at decision t holds what was played at t
    n_rows = 0
    for a in range(N6 - 1):
        for r in b.replay_rows(a):
            t, i = int(r["tick_prev"]), int(r["ship"])
            assert (int(r["iaction"]), int(r["px"]), int(r["py"])) == (int(played[t]["thrust"][a, i]), int(played[t]["px"][a, i]),
                                                                     int(played[t]["py"][a, i]))
            n_rows += 1
    assert n_rows >= 2 * (N6 - 1) * 2 and len(b.replay_rows(N6 - 1)) == 0
    b.close()
    del b, tr, roll
    # restored into fresh objects: the same weights and rows, bit for bit
    b, tr, roll = _build6()
    man = roll.restore(path)
    assert man["rollout_fingerprint"]["boltzmann"] == list(TAU6)
    after = _state6(b, tr)
    assert [k for k in after if after[k] != mid[k]] == []
    roll.run(STEPS6 - 4)
    got = _state6(b, tr)
    assert [k for k in got if got[k] != end[k]] == []
    b.close()
