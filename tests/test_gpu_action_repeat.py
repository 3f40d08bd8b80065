"""Action repeat on the device: ofx_step_repeat against the sequential composition it stands for and against the CPU
model (tests/repeat_oracle.py), its maps, the replay memory's reward source, and TrainingRollout(action_repeat=K) end to
end and through a checkpoint."""
import ctypes as C

import numpy as np
import pytest

from tests import repeat_oracle as ro
from tests.actor_priority_oracle import ArenaOracle, within_2ulp

pytestmark = pytest.mark.gpu

N, W, H = ro.N, ro.W, ro.H


def _batch(m=ro.M, seed=ro.SEED):
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, m, **ro.REWARDS)
    b.spawn_random(seed)
    return b


SHIP_FIELDS = ("F_SHIP_X", "F_SHIP_Y", "F_SHIP_PX", "F_SHIP_PY", "F_SHIP_ALIVE", "F_HULL", "F_REWARD", "F_OBS_REWARD",
               "F_SCORE", "F_KILLER")
LASER_FIELDS = ("F_LASER_X", "F_LASER_Y", "F_LASER_DX", "F_LASER_DY", "F_LASER_OWNER", "F_LASER_DEAD")


def _state(b):
    """Every ship field, n_lasers and the live prefix of all laser arrays."""
    from ofighters_amd import _native as nat
    s = {f: b.get(getattr(nat, f)) for f in SHIP_FIELDS}
    n = b.get(nat.F_N_LASERS)
    s["n_lasers"] = n
    for f in LASER_FIELDS:
        full = b.get(getattr(nat, f))
        s[f] = [full[g, :n[g]].copy() for g in range(b.N)]
    return s


def _differences(x, y):
    bad = []
    for k in x:
        same = (all(np.array_equal(p, q) for p, q in zip(x[k], y[k])) if isinstance(x[k], list)
                else np.array_equal(x[k], y[k]))
        if not same:
            bad.append(k)
    return bad


def _pack(act5):
    from ofighters_amd.engine import pack_actions
    return pack_actions(act5[..., 0], act5[..., 1], act5[..., 2], act5[..., 3], act5[..., 4])


def _sequential_span(b, behaviours, seed, tick0, k, held_actions, held):
    """k x (bot_actions(tick0 + j), the held ships' entries overwritten, step) -> the summed F_REWARD, int64 [N][M]."""
    from ofighters_amd import _native as nat
    total = np.zeros((b.N, b.M), np.int64)
    for j in range(k):
        b.bot_actions(behaviours, seed, tick=tick0 + j)
        act = b.actions_host()
        for i in held:
            act[:, i] = held_actions[:, i]
        b.step(act)
        total += b.get(nat.F_REWARD)
    return total


class _Held:
    """The device side of a set of held ships: the mask, an action array and the span-reward buffer."""

    def __init__(self, b, held):
        from ofighters_amd import DeviceBuffer
        from ofighters_amd.engine import ACTION_DTYPE
        mk = np.zeros((b.N, b.M), np.uint8)
        mk[:, list(held)] = 1
        self.b, self.held = b, tuple(held)
        self.mask = DeviceBuffer(mk.nbytes).upload(mk)
        self.actions = DeviceBuffer(b.N * b.M * ACTION_DTYPE.itemsize)
        self.span = DeviceBuffer(4 * b.N * b.M).upload(np.full((b.N, b.M), -77, np.int32))   # every entry is written

    def span_host(self):
        self.b.sync()
        return self.span.download(np.int32, (self.b.N, self.b.M))

    def step_repeat(self, behaviours, seed, tick0, k, packed, observe=None):
        self.b.sync()                                            # raw copies are not ordered with the handle's stream
        self.actions.upload(packed)
        self.b.step_repeat(behaviours, seed, tick0, k, self.mask.ptr, self.actions.ptr, self.span.ptr, observe)


# ----------------------------------------------------------------------- 1. step_repeat == the sequential composition
CASES = {
    "K1": dict(k=1, spans=12), "K2": dict(k=2, spans=12), "K4": dict(), "K7": dict(k=7, spans=8),
    "M13": dict(m=13, behaviours=["random"] * 7 + ["turret"] * 6, held=(0, 12), k=3, spans=10),
    "restart": dict(restart_after=5),
}


@pytest.mark.parametrize("case", list(CASES))
def test_step_repeat_is_the_sequential_composition(case):
    from ofighters_amd import _native as nat
    kw = CASES[case]
    sc = ro.scenario(**kw)
    m, beh, held = kw.get("m", ro.M), kw.get("behaviours", ro.BEHAVIOURS), kw.get("held", ro.HELD)
    k, spans, restart_after = kw.get("k", ro.K), kw.get("spans", ro.SPANS), kw.get("restart_after")
    a, b = _batch(m), _batch(m)                                  # a: step_repeat, b: the sequential twin
    ha = _Held(a, held)
    for s in range(spans):
        alive = a.get(nat.F_SHIP_ALIVE)
        assert np.array_equal(alive, sc["alive0"][s]), (case, s, "alive at the decision")
        packed = _pack(sc["actions"][s])
        ha.step_repeat(beh, ro.SEED, s * k, k, packed)
        want_span = _sequential_span(b, beh, ro.SEED, s * k, k, packed, held)
        assert a.tick == b.tick == (s + 1) * k
        assert _differences(_state(a), _state(b)) == [], (case, s)
        got_span = ha.span_host()
        assert np.array_equal(got_span, want_span), (case, s, "span_reward")
        assert np.array_equal(got_span, sc["rewards"][s].sum(axis=0)), (case, s, "span_reward against the model")
        if restart_after is not None and s == restart_after:
            a.restart_random(ro.SEED), b.restart_random(ro.SEED)
    st = _state(a)
    for g in range(N):                                           # the CPU model's final state
        o, l = sc["ships"][g], sc["lasers"][g]
        assert np.array_equal(np.stack([st["F_SHIP_X"][g], st["F_SHIP_Y"][g]], 1), o["xy"]), (case, g)
        assert np.array_equal(np.stack([st["F_SHIP_PX"][g], st["F_SHIP_PY"][g]], 1), o["pt"]), (case, g)
        for f, key in (("F_SHIP_ALIVE", "alive"), ("F_REWARD", "reward"), ("F_SCORE", "score"), ("F_KILLER", "killer"),
                       ("F_HULL", "hull")):
            assert np.array_equal(st[f][g], o[key]), (case, g, f)
        assert st["n_lasers"][g] == len(l["x"])
        assert np.array_equal(st["F_LASER_X"][g], l["x"]) and np.array_equal(st["F_LASER_Y"][g], l["y"]), (case, g)
        assert np.array_equal(st["F_LASER_OWNER"][g], l["owner"]) and np.array_equal(st["F_LASER_DEAD"][g], l["destroyed"])
    assert a.overflow_count() == 0 and b.overflow_count() == 0
    a.close(), b.close()


def test_step_repeat_errors():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    b = ArenaBatch(N, ro.M)
    with pytest.raises(OfxError) as err:
        b.step_repeat(ro.BEHAVIOURS, 1, 0, 2)
    assert err.value.code == nat.OFX_ERR_STATE
    b.spawn_random(1)
    h = _Held(b, ro.HELD)
    beh = np.zeros(ro.M, np.int32)
    call = lambda hh, bp, n, mask, act: nat.lib().ofx_step_repeat(hh, bp, 1, 0, n, mask, act, None, -1)
    bp = beh.ctypes.data_as(C.c_void_p)
    assert call(None, bp, 2, None, None) == nat.OFX_ERR_INVALID
    assert call(b.handle, None, 2, None, None) == nat.OFX_ERR_INVALID
    assert call(b.handle, bp, 0, None, None) == nat.OFX_ERR_INVALID
    assert call(b.handle, bp, 2, h.mask.ptr, None) == nat.OFX_ERR_INVALID
    assert b.tick == 0 and (b.get(nat.F_TIME) == 0).all()        # nothing ran
    b.close()


# -------------------------------------------------------------------------------------------------- 2. hold_mask = None
def test_no_mask_is_the_headless_rollout():
    a, b = _batch(), _batch()
    t = 0
    for k in (1, 5, 3, 6):
        a.step_repeat(ro.BEHAVIOURS, ro.SEED, t, k)
        b.rollout(ro.BEHAVIOURS, ro.SEED, t, k)
        t += k
        assert a.tick == b.tick == t
        assert _differences(_state(a), _state(b)) == [], k
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------------ 3. observation
def _maps_raw(b, map_type):
    """The handle's maps of map_type as they lie there (maps_host would rasterise them again)."""
    from ofighters_amd import _native as nat
    from ofighters_amd.engine import _MAP_DTYPE
    per = nat.lib().ofx_map_bytes(b.handle, map_type)
    b.sync()
    out = []
    for which in (0, 1):
        m = np.empty((b.N, per), np.uint8)
        nat.check(nat.lib().ofx_memcpy_d2h(m.ctypes.data_as(C.c_void_p), nat.lib().ofx_map_ptr(b.handle, map_type, which),
                                           m.nbytes))
        out.append(m.view(_MAP_DTYPE[map_type]))
    return out


@pytest.mark.parametrize("map_type", ["MAP_BITS", "MAP_U8"])
def test_maps_after_a_span_are_the_last_steps(map_type):
    from ofighters_amd import _native as nat
    mt = getattr(nat, map_type)
    sc = ro.scenario()
    a, b = _batch(), _batch()
    ha = _Held(a, ro.HELD)
    destroyed_on_last = 0
    for s in range(ro.SPANS):
        packed = _pack(sc["actions"][s])
        ha.step_repeat(ro.BEHAVIOURS, ro.SEED, s * ro.K, ro.K, packed, observe=mt)
        got = _maps_raw(a, mt)
        _sequential_span(b, ro.BEHAVIOURS, ro.SEED, s * ro.K, ro.K, packed, ro.HELD)
        want = b.maps_host(mt)
        for which in (0, 1):
            assert np.array_equal(got[which].reshape(N, -1), want[which].reshape(N, -1)), (s, which)
        assert want[0].any() and want[1].any()
        # a laser destroyed on the span's last lock-step is still listed (and drawn) until the next lock-step clears it
        n, dead = b.get(nat.F_N_LASERS), b.get(nat.F_LASER_DEAD)
        destroyed_on_last += int(any(dead[g, :n[g]].any() for g in range(N)))
    assert destroyed_on_last >= 1
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------- 4. reward source
CAP, ALPHA, EPS, GAMMA = 16, 0.6, 1e-3, 0.9
DECISIONS, SOURCE_OFF_AT = 14, 12


class _Latches:
    """QlearnIA.play's bookkeeping for the capturing ships: who plays and whose row completes at a capture."""

    def __init__(self, mask):
        self.mask = mask
        self.latched, self.has_prev = np.zeros_like(mask), np.zeros_like(mask)

    def step(self, done):
        plays = self.mask & ~self.latched
        has_row = plays & self.has_prev
        self.latched |= plays & (done != 0)
        self.has_prev |= plays
        return plays, has_row


def test_reward_source():
    """14 decisions with step_repeat K = 4 between them on the scenario of the CPU test (12 of them under the reward
    source, then two without), explicit iaction / ipointer; a plain memory and a prioritized one with actor priorities."""
    from ofighters_amd import DeviceBuffer, OfxError, _native as nat
    sc = ro.scenario(spans=DECISIONS)
    S = N * ro.M
    a, v = _batch(), _batch()                                    # a: ofx_replay_capture, v: ofx_replay_capture_valued
    with pytest.raises(OfxError) as err:
        a.replay_reward_source(None)
    assert err.value.code == nat.OFX_ERR_STATE                   # no replay memory yet
    for b in (a, v):
        b.replay_create(CAP, 0)
    v.replay_prioritize(ALPHA, EPS)
    v.replay_actor_priorities(GAMMA)
    ha, hv = _Held(a, ro.HELD), _Held(v, ro.HELD)
    for b, h in ((a, ha), (v, hv)):
        b.sync()
        h.span.upload(np.zeros((N, ro.M), np.int32))
        b.replay_reward_source(h.span.ptr)
    mask = np.zeros((N, ro.M), bool)
    mask[:, list(ro.HELD)] = True
    lat = _Latches(mask)
    ora = [ArenaOracle(ro.M, CAP, ALPHA, EPS, GAMMA) for _ in range(N)]
    rs = np.random.RandomState(5)
    ia_d, ip_d = DeviceBuffer(4 * S), DeviceBuffer(8 * S)
    vals_d = [DeviceBuffer(4 * S) for _ in range(4)]
    want_rows = [[] for _ in range(N)]                           # (ship, tick_next, reward, head_next[0])
    for d in range(DECISIONS):
        if d == SOURCE_OFF_AT:
            a.replay_reward_source(None), v.replay_reward_source(None)
        head, done = a.observe_head()                            # head[..., 0]: the state's reward
        span = ha.span_host()
        assert np.array_equal(span, hv.span_host())
        if d:
            assert np.array_equal(span, sc["rewards"][d - 1].sum(axis=0))
        row_reward = span if d < SOURCE_OFF_AT else head[..., 0].astype(np.int64)
        plays, has_row = lat.step(done)
        ia = rs.randint(0, 2, (N, ro.M)).astype(np.int32)
        ip = np.stack([rs.randint(0, W, (N, ro.M)), rs.randint(0, H, (N, ro.M))], -1).astype(np.int32)
        vals = [(3.0 * rs.standard_normal((N, ro.M))).astype(np.float32) for _ in range(4)]     # q_sa, p_sp, v_act, v_ptr
        a.sync(), v.sync()
        ia_d.upload(ia), ip_d.upload(ip)
        for buf, x in zip(vals_d, vals):
            buf.upload(x)
        a.replay_capture(d, ha.mask.ptr, ia_d.ptr, ip_d.ptr)
        v.replay_capture_valued(d, hv.mask.ptr, ia_d.ptr, ip_d.ptr, *[x.ptr for x in vals_d])
        for g in range(N):
            ora[g].capture_valued(row_reward[g], done[g], has_row[g], plays[g], *[x[g] for x in vals])
            want_rows[g] += [(i, d, int(row_reward[g, i]), float(head[g, i, 0])) for i in range(ro.M) if has_row[g, i]]
        packed = _pack(sc["actions"][d])
        ha.step_repeat(ro.BEHAVIOURS, ro.SEED, d * ro.K, ro.K, packed)
        hv.step_repeat(ro.BEHAVIOURS, ro.SEED, d * ro.K, ro.K, packed)
    a.sync(), v.sync()
    sum_is_not_state = off_rows = 0
    for g in range(N):
        rows = a.replay_rows(g)
        want = want_rows[g][-CAP:]
        assert len(rows) == len(want) and len(rows) > 0
        assert rows.tobytes() == v.replay_rows(g).tobytes()      # the valued form stores the same rows
        for r, (ship, tick_next, reward, head0) in zip(rows, want):
            assert (r["ship"], r["tick_next"], r["tick_prev"]) == (ship, tick_next, tick_next - 1)
            assert r["reward"] == reward, (g, ship, tick_next)
            assert r["head_next"][0] == np.float32(head0), (g, ship, tick_next)      # the state's reward, always
            if tick_next >= SOURCE_OFF_AT:
                off_rows += 1
                assert r["reward"] == r["head_next"][0]          # source off: the state's reward again
            else:
                sum_is_not_state += int(r["reward"] != r["head_next"][0])
        got = v.replay_priorities(g)
        assert within_2ulp(got, list(ora[g].mass)), (g, got, list(ora[g].mass))
    assert sum_is_not_state >= 3 and off_rows >= 3
    a.close(), v.close()


# ------------------------------------------------------------------------------------------------------- 5. end to end
DEC = 25


def _build(trainer_kw=None, **roll_kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N, ro.M, **ro.REWARDS)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=32, fit_batch=8,
                       **(trainer_kw or {}))
    roll = TrainingRollout(b, tr, ro.BEHAVIOURS, ro.SEED, policy_ships=(0,), episode_ticks=40, collecting_steps=3,
                           replay_every=2, action_repeat=4, **roll_kw)
    return b, tr, roll


def test_training_rollout_with_action_repeat():
    from ofighters_amd import _native as nat
    b, tr, roll = _build()
    twin = _batch()
    spans = []                                                   # per decision: the twin's span sums [N][M]
    for d in range(DEC):
        if roll.tick > 0 and roll.tick % 40 == 0:
            twin.restart_random(ro.SEED)
        t0 = roll.tick
        roll.lockstep()
        assert roll.tick == t0 + 4 and b.tick == roll.tick and roll.total_steps == d + 1 and roll.capture_tick == d + 1
        held = b.actions_host()                                  # step_repeat does not write the action array
        spans.append(_sequential_span(twin, ro.BEHAVIOURS, ro.SEED, t0, 4, held, (0,)))
        assert _differences(_state(b), _state(twin)) == [], d
        assert np.array_equal(roll._span.download(np.int32, (N, ro.M)), spans[-1]), d
    assert roll.episode == 2 and tr.fit_steps >= 5 and np.isfinite(roll.losses).all()
    n_rows = nonzero = not_state = 0
    for g in range(N):
        for r in b.replay_rows(g):
            assert r["ship"] == 0 and r["tick_next"] - r["tick_prev"] == 1
            assert r["reward"] == spans[r["tick_prev"]][g, 0], (g, r["tick_prev"])
            n_rows += 1
            nonzero += int(r["reward"] != 0)
            not_state += int(r["reward"] != r["head_next"][0])
    assert n_rows >= N * 10 and nonzero >= 3 and not_state >= 1
    assert b.overflow_count() == 0
    b.close(), twin.close()


def test_training_rollout_with_action_repeat_nstep_per_actor():
    b, tr, roll = _build(dict(n_step=3, prioritized=True, actor_priorities=True))
    roll.run(DEC)
    assert roll.tick == 4 * DEC and tr.fit_steps >= 5 and len(roll.losses) >= 5 and np.isfinite(roll.losses).all()
    b.close()


# --------------------------------------------------------------------------------------------------------- 6. checkpoint
def _train_state(b, tr, roll):
    b.sync()
    s = {"weights": tr.weights_host().tobytes(), "adam_m": tr.adam_m.download(np.float32, (tr.n_floats,)).tobytes(),
         "adam_v": tr.adam_v.download(np.float32, (tr.n_floats,)).tobytes(), "losses": list(tr.losses),
         "roll_losses": list(roll.losses), "fit_steps": tr.fit_steps, "epsilon": tr.epsilon.get(),
         "counters": (roll.tick, roll.total_steps, roll.capture_tick, roll.episode, b.episode, b.tick),
         "span": roll._span.download(np.int32, (N, ro.M)).tobytes(),
         "rows": [b.replay_rows(g).tobytes() for g in range(N)],
         "count": [x.tobytes() for x in b.replay_count()]}
    for f in range(19):
        s["field%d" % f] = b.get(f).tobytes()
    return s


def test_checkpoint_resume_is_bit_identical(tmp_path):
    b, tr, roll = _build()
    roll.run(12)
    mid = _train_state(b, tr, roll)
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    roll.run(13)
    end = _train_state(b, tr, roll)
    assert end["fit_steps"] >= mid["fit_steps"] + 3 and np.frombuffer(mid["span"], np.int32).any()
    b.close()
    del b, tr, roll
    b, tr, roll = _build()
    m = roll.restore(path)
    assert m["rollout_fingerprint"]["action_repeat"] == 4 and m["counters"]["tick"] == 48
    assert m["sections"]["rollout/span_reward"]["shape"] == [N, ro.M]
    after = _train_state(b, tr, roll)
    assert [k for k in after if after[k] != mid[k]] == []
    roll.run(13)
    got = _train_state(b, tr, roll)
    assert [k for k in got if got[k] != end[k]] == []            # names what differs; every entry is compared with ==
    b.close()
