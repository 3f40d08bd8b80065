"""Actor-side initial priorities on the device: ofx_policy_act against the two calls it stands for, the valued capture
against a twin handle running the plain capture (rows, frames) and tests/actor_priority_oracle.py (masses, running
maximum), the rollout with the option on and off, and a checkpoint that carries the ships' previous values."""
import numpy as np
import pytest

from tests.actor_priority_oracle import ArenaOracle, within_2ulp

pytestmark = pytest.mark.gpu

W = H = 400
SEED = 0x0F160031
ALPHA, EPS, GAMMA = 0.6, 1e-3, 0.9
SENTINEL = np.float32(-12345.0)


def _f32(n):
    from ofighters_amd import DeviceBuffer
    return DeviceBuffer(4 * n)


class _Latches:
    """QlearnIA.play's bookkeeping per ship, kept by the test: which ships play and which complete a row."""

    def __init__(self, mask):
        self.mask = np.asarray(mask, bool)
        self.reset()

    def reset(self):
        self.has_prev = np.zeros(self.mask.shape, bool)
        self.latched = np.zeros(self.mask.shape, bool)

    def step(self, done):
        plays = self.mask & ~self.latched
        has_row = plays & self.has_prev
        self.latched |= plays & (np.asarray(done) != 0)
        self.has_prev |= plays
        return plays, has_row


def _memory(b, ticks):
    """Rows, counts and every held frame of a handle, in comparable form."""
    from ofighters_amd import OfxError, _native as nat
    cnt, app = b.replay_count()
    frames = []
    for a in range(b.N):
        held = {}
        for t in range(ticks):
            try:
                s, l = b.replay_frame(a, t)
                held[t] = (np.packbits(s).tobytes(), np.packbits(l).tobytes())
            except OfxError as err:                        # the one expected refusal: the ring does not hold the frame
                assert err.code == nat.OFX_ERR_STATE and "not in the frame ring" in str(err), str(err)
        frames.append(held)
    return cnt.tobytes(), app.tobytes(), [b.replay_rows(a).tobytes() for a in range(b.N)], frames


# ------------------------------------------------------------------------------ 1. act == forward + explore
def test_act_equals_forward_plus_explore():
    """3 arenas x 2 ships with ship 1 of arena 0 and ship 0 of arena 1 left out: the compacted list index of every later
    ship differs from its ship index a * M + i."""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    N, M = 3, 2
    S = N * M
    mask = np.array([[1, 0], [0, 1], [1, 1]], np.uint8)
    a, b = ArenaBatch(N, M), ArenaBatch(N, M)
    a.spawn_random(SEED), b.spawn_random(SEED)
    w = synthetic(7)
    dw, dm = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(mask.nbytes).upload(mask)
    vals = [_f32(S) for _ in range(4)]
    act_d, ia_d, ip_d, heat_d = _f32(2 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S), _f32(S * W * H)
    sel = mask.astype(bool)
    explored = greedy = 0
    for tick, collecting in ((0, 0), (1, 0), (2, 0), (3, 0), (4, 1)):
        a.sync()
        for v in vals:
            v.upload(np.full(S, SENTINEL, np.float32))
        for e in (a, b):
            e.bot_actions(["random"] * M, SEED, tick=tick)
        a.policy_act(dw.ptr, 0.5, SEED, tick=tick, collecting=collecting, ship_mask_ptr=dm.ptr, q_sa_ptr=vals[0].ptr,
                     p_sp_ptr=vals[1].ptr, v_act_ptr=vals[2].ptr, v_ptr_ptr=vals[3].ptr)
        a.policy_actions(ship_mask_ptr=dm.ptr)
        # the two calls ofx_policy_act stands for, results kept by the handle
        b.policy_forward(dw.ptr, dm.ptr)
        b.policy_explore(0.5, SEED, tick=tick, collecting=collecting, ship_mask_ptr=dm.ptr)
        b.policy_actions(ship_mask_ptr=dm.ptr)
        got, want = a.actions_host(), b.actions_host()
        assert got.tobytes() == want.tobytes()
        # the whole forward, into buffers of the test (the handle's results stay)
        b.policy_forward(dw.ptr, dm.ptr, act_d.ptr, ia_d.ptr, ip_d.ptr, heat_d.ptr)
        b.sync()
        act = act_d.download(np.float32, (N, M, 2))
        heat = heat_d.download(np.float32, (N, M, W, H))
        arg = ip_d.download(np.int32, (N, M, 2))
        q_sa, p_sp, v_act, v_ptr = (v.download(np.float32, (N, M)) for v in vals)
        for g in range(N):
            for i in range(M):
                if not sel[g, i]:
                    continue
                ia, px, py = int(want["thrust"][g, i]), int(want["px"][g, i]), int(want["py"][g, i])
                assert want["shoot"][g, i] == 1 - ia
                assert q_sa[g, i] == act[g, i, ia], (tick, g, i)
                assert v_act[g, i] == act[g, i].max()
                assert v_ptr[g, i] == heat[g, i].max()
                assert p_sp[g, i] == heat[g, i, py, px], (tick, g, i, px, py)
                if (px, py) == tuple(arg[g, i]):
                    greedy += not collecting
                else:
                    explored += 1
        for v in (q_sa, p_sp, v_act, v_ptr):
            assert (v[~sel] == SENTINEL).all()
        a.step(), b.step()
    assert explored >= 4 and greedy >= 1, (explored, greedy)        # epsilon = 0.5 drew both kinds; the last tick collects
    a.close(), b.close()


# ------------------------------------------------------------------------------ 2. valued capture vs the oracle
N2, M2, CAP2 = 2, 3, 4
# ship 0 shoots at ship 1, which stands 40 (arena 0) / 70 (arena 1) pixels away and dies after a few lock-steps
SPAWN2 = np.array([[[100, 100], [140, 100], [300, 300]], [[100, 100], [170, 100], [300, 300]]], np.int32)


def _scripted_step(b):
    from ofighters_amd import pack_actions
    one = np.ones((N2, M2), np.int32)
    shoot = np.zeros((N2, M2), np.int32)
    shoot[:, 0] = 1
    px = np.broadcast_to(SPAWN2[:, 1:2, 0], (N2, M2))
    py = np.broadcast_to(SPAWN2[:, 1:2, 1], (N2, M2))
    b.step(pack_actions(one, shoot, 0 * one, px, py))


def _fresh2(valued):
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N2, M2)
    b.spawn(SPAWN2)
    b.replay_create(CAP2, 0)
    b.replay_prioritize(ALPHA, EPS)
    if valued:
        b.replay_actor_priorities(GAMMA)
    return b


def test_valued_capture_against_the_oracle():
    from ofighters_amd import DeviceBuffer
    S = N2 * M2
    a, b = _fresh2(True), _fresh2(False)                     # b: the twin running the plain capture
    lat = _Latches(np.ones((N2, M2), bool))
    ora = [ArenaOracle(M2, CAP2, ALPHA, EPS, GAMMA) for _ in range(N2)]
    rs = np.random.RandomState(11)
    ia_d, ip_d = DeviceBuffer(4 * S), DeviceBuffer(8 * S)
    vals_d = [_f32(S) for _ in range(4)]
    T, RESTART, NAN_AT = 12, 8, 5
    done_rows = rows_after_restart = 0
    for t in range(T):
        if t == RESTART:
            a.restart(SPAWN2), b.restart(SPAWN2)
            lat.reset()
        head, done = a.observe_head()
        ia = rs.randint(0, 2, (N2, M2)).astype(np.int32)
        ip = np.stack([rs.randint(0, W, (N2, M2)), rs.randint(0, H, (N2, M2))], -1).astype(np.int32)
        vals = [(3.0 * rs.standard_normal((N2, M2))).astype(np.float32) for _ in range(4)]     # q_sa, p_sp, v_act, v_ptr
        plays, has_row = lat.step(done)
        if t == NAN_AT:
            assert has_row[0, 0] and not done[0, 0]
            vals[3][0, 0] = np.nan
        done_rows += int((has_row & (done != 0)).sum())
        rows_after_restart += int(has_row.sum()) if t > RESTART else 0
        if t == RESTART:
            assert not has_row.any()                        # has_prev was cleared: no row, the stale prev_q is not used
        a.sync(), b.sync()
        ia_d.upload(ia), ip_d.upload(ip)
        for d, v in zip(vals_d, vals):
            d.upload(v)
        a.replay_capture_valued(t, None, ia_d.ptr, ip_d.ptr, *[d.ptr for d in vals_d])
        b.replay_capture(t, None, ia_d.ptr, ip_d.ptr)
        for g in range(N2):
            ora[g].capture_valued(head[g, :, 0], done[g], has_row[g], plays[g], *[v[g] for v in vals])
        _scripted_step(a), _scripted_step(b)
    a.sync(), b.sync()
    assert done_rows >= 2 and rows_after_restart >= 3 and ora[0].fallbacks == 1
    _, app, _, _ = _memory(a, T)
    assert np.frombuffer(app, np.int64).min() > CAP2        # the ring wrapped: masses landed at (head + pos) % C
    assert _memory(a, T) == _memory(b, T)                   # rows and frame bookkeeping: byte-identical to the plain capture
    for g in range(N2):
        got = a.replay_priorities(g)
        assert within_2ulp(got, list(ora[g].mass)), (g, got, list(ora[g].mass))
        assert (b.replay_priorities(g) == 1.0).all()
        assert len(set(got.tolist())) > 1
    prev_q = a.replay_actor_values()
    assert np.array_equal(prev_q, np.stack([o.prev_q for o in ora]))
    # the running maximum, read through one plain capture on the enabled handle: its rows enter at mmax[a], prev_q stays
    head, done = a.observe_head()
    plays, has_row = lat.step(done)
    assert has_row.any(axis=1).all()
    a.replay_capture(T, None, ia_d.ptr, ip_d.ptr)
    a.sync()
    for g in range(N2):
        k = int(has_row[g].sum())
        got = a.replay_priorities(g)
        assert len(set(got[-k:].tolist())) == 1 and within_2ulp(got[-1], ora[g].mmax), (g, got, ora[g].mmax)
        assert ora[g].mmax > 1.0
    assert np.array_equal(a.replay_actor_values(), prev_q)
    a.close(), b.close()


# ------------------------------------------------------------------------------ 3. the handle's values, error codes
def test_null_values_are_the_last_acts_and_error_codes():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    from ofighters_amd.agents.policy_weights import synthetic
    N, M, cap = 2, 2, 16
    S = N * M
    w = synthetic(7)
    dw = DeviceBuffer(w.nbytes).upload(w)

    def fresh(per=True, actor=True):
        e = ArenaBatch(N, M)
        e.spawn_random(SEED)
        e.replay_create(cap, 0)
        if per:
            e.replay_prioritize(ALPHA, EPS)
        if actor:
            e.replay_actor_priorities(GAMMA)
        return e

    a, b = fresh(), fresh()
    vals = [_f32(S) for _ in range(4)]
    ptrs = [v.ptr for v in vals]
    # before any ofx_policy_act: no values to fall back on
    with pytest.raises(OfxError) as err:
        a.replay_capture_valued(0)
    assert err.value.code == nat.OFX_ERR_STATE
    with pytest.raises(OfxError) as err:
        a.replay_capture_valued(0, None, None, None, ptrs[0], ptrs[1], ptrs[2], None)      # three of four
    assert err.value.code == nat.OFX_ERR_INVALID
    for t in range(5):
        for e in (a, b):
            e.bot_actions(["random"] * M, SEED, tick=t)
        a.policy_act(dw.ptr, 0.3, SEED, tick=t)
        a.replay_capture_valued(t)
        b.policy_act(dw.ptr, 0.3, SEED, tick=t, q_sa_ptr=ptrs[0], p_sp_ptr=ptrs[1], v_act_ptr=ptrs[2], v_ptr_ptr=ptrs[3])
        b.replay_capture_valued(t, None, None, None, *ptrs)
        for e in (a, b):
            e.policy_actions()
            e.step()
    a.sync(), b.sync()
    assert _memory(a, 5) == _memory(b, 5)
    masses = [a.replay_priorities(g) for g in range(N)]
    for g in range(N):
        assert masses[g].tobytes() == b.replay_priorities(g).tobytes()          # bit for bit
        assert len(masses[g]) >= M and np.isfinite(masses[g]).all() and len(set(masses[g].tolist())) > 1
    assert np.array_equal(a.replay_actor_values(), b.replay_actor_values())
    # plain capture on the enabled handle: the new rows take mmax[a] = the largest mass so far (nothing was evicted)
    a.policy_act(dw.ptr, 0.3, SEED, tick=5)
    a.replay_capture(5)
    a.sync()
    for g in range(N):
        got = a.replay_priorities(g)
        k = len(got) - len(masses[g])
        assert k >= 1 and got[:-k].tobytes() == masses[g].tobytes()
        assert (got[-k:] == max(np.float32(1.0), masses[g].max())).all()
    a.close(), b.close()
    # the entry points' state and argument checks
    c = fresh(per=False, actor=False)
    with pytest.raises(OfxError) as err:
        c.replay_actor_priorities(GAMMA)                    # needs ofx_replay_prioritize
    assert err.value.code == nat.OFX_ERR_STATE
    c.replay_prioritize(ALPHA, EPS)
    for call in (lambda: c.replay_capture_valued(0, None, None, None, *ptrs), c.replay_actor_values,
                 lambda: c.set_replay_actor_values(np.zeros((N, M, 2), np.float32))):
        with pytest.raises(OfxError) as err:
            call()                                          # actor priorities are not enabled
        assert err.value.code == nat.OFX_ERR_STATE
    for gamma in (-0.1, 1.5, float("nan")):
        with pytest.raises(OfxError) as err:
            c.replay_actor_priorities(gamma)
        assert err.value.code == nat.OFX_ERR_INVALID
    c.replay_actor_priorities(1.0)
    # an ofx_policy_act with explicit outputs leaves nothing in the handle for a capture without values
    c.policy_act(dw.ptr, 0.3, SEED, tick=0)
    c.policy_act(dw.ptr, 0.3, SEED, tick=0, q_sa_ptr=ptrs[0], p_sp_ptr=ptrs[1], v_act_ptr=ptrs[2], v_ptr_ptr=ptrs[3])
    with pytest.raises(OfxError) as err:
        c.replay_capture_valued(0)
    assert err.value.code == nat.OFX_ERR_STATE
    v = np.arange(N * M * 2, dtype=np.float32).reshape(N, M, 2)
    c.set_replay_actor_values(v)
    assert np.array_equal(c.replay_actor_values(), v)
    with pytest.raises(OfxError) as err:                    # epsilon is checked like ofx_policy_explore checks it
        c.policy_act(dw.ptr, 1.5, SEED, tick=0)
    assert err.value.code == nat.OFX_ERR_INVALID
    c.close()


# ------------------------------------------------------------------------------ 4. the rollout, option on and off
N4, M4, STEPS4 = 4, 3, 25


def _build4(actor, n=N4):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(n, M4)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), epsilon=eps, memory_size=32, fit_batch=16, prioritized=True, per_alpha=ALPHA,
                       per_eps=EPS, actor_priorities=actor)
    roll = TrainingRollout(b, tr, ["random"] * M4, SEED, policy_ships=(0,), collecting_steps=10, replay_every=0,
                           replay_on_death=False)
    return b, tr, roll


def test_rollout_plays_the_same_and_primes_the_priorities():
    from ofighters_amd import DeviceBuffer
    runs = {}
    for actor in (False, True):
        b, tr, roll = _build4(actor)
        actions = []
        for _ in range(STEPS4):
            roll.lockstep()
            actions.append(b.actions_host().tobytes())
        b.sync()
        runs[actor] = dict(actions=actions, memory=_memory(b, STEPS4), state=[b.get(f).tobytes() for f in range(19)],
                           mass=[b.replay_priorities(g) for g in range(N4)], weights=tr.weights_host().tobytes(),
                           prev_q=b.replay_actor_values() if actor else None, eps=tr.epsilon.get())
        b.close()
    off, on = runs[False], runs[True]
    for k in ("actions", "memory", "state", "weights", "eps"):
        assert on[k] == off[k], k
    assert all((m == 1.0).all() and len(m) >= 1 for m in off["mass"])
    allm = np.concatenate(on["mass"])
    assert np.isfinite(allm).all() and (allm > 0).all() and len(set(allm.tolist())) > 1
    # the same lock-steps driven by hand on a twin handle, explicit buffers, the oracle fed with what came back
    b, tr, roll = _build4(True)
    S = N4 * M4
    mask = roll.policy_mask.astype(bool)
    lat = _Latches(mask)
    ora = [ArenaOracle(M4, 32, ALPHA, EPS, tr.gamma) for _ in range(N4)]
    vals_d = [_f32(S) for _ in range(4)]
    ptrs = [d.ptr for d in vals_d]
    m = roll._mask.ptr
    for t in range(STEPS4):
        collecting = t + 1 < roll.collecting_steps
        b.bot_actions(["random"] * M4, SEED, tick=t)
        head, done = b.observe_head()
        b.policy_act(tr.weights.ptr, tr.epsilon.get(), SEED, tick=t, collecting=collecting, ship_mask_ptr=m,
                     q_sa_ptr=ptrs[0], p_sp_ptr=ptrs[1], v_act_ptr=ptrs[2], v_ptr_ptr=ptrs[3])
        b.replay_capture_valued(t, m, None, None, *ptrs)
        b.policy_actions(ship_mask_ptr=m)
        b.sync()
        vals = [d.download(np.float32, (N4, M4)) for d in vals_d]
        plays, has_row = lat.step(done)
        for g in range(N4):
            ora[g].capture_valued(head[g, :, 0], done[g], has_row[g], plays[g], *[v[g] for v in vals])
        if not collecting:
            tr.decay_epsilon()
        b.step()
        b.rasterise()
    b.sync()
    assert _memory(b, STEPS4) == on["memory"]
    for g in range(N4):
        assert b.replay_priorities(g).tobytes() == on["mass"][g].tobytes()
        assert within_2ulp(on["mass"][g], list(ora[g].mass)), (g, on["mass"][g], list(ora[g].mass))
    assert np.array_equal(b.replay_actor_values(), on["prev_q"])
    assert np.array_equal(on["prev_q"], np.stack([o.prev_q for o in ora]))
    b.close()


# ------------------------------------------------------------------------------ 5. checkpoint
def _build5(actor):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(2, M4)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=8,
                       prioritized=True, actor_priorities=actor)
    roll = TrainingRollout(b, tr, ["random"] * M4, SEED, policy_ships=(0, 1), episode_ticks=20, collecting_steps=3,
                           replay_every=3)
    return b, tr, roll


def _state5(b, tr):
    b.sync()
    return dict(weights=tr.weights_host().tobytes(), mass=[b.replay_priorities(g).tobytes() for g in range(b.N)],
                prev_q=b.replay_actor_values().tobytes(), fit_steps=tr.fit_steps, memory=_memory(b, 40))


def test_checkpoint_carries_the_actor_values(tmp_path):
    path, path_off = str(tmp_path / "on"), str(tmp_path / "off")
    b, tr, roll = _build5(True)
    roll.run(12)
    assert tr.fit_steps >= 3
    mid = _state5(b, tr)
    assert np.frombuffer(mid["prev_q"], np.float32).any()
    roll.checkpoint(path)
    roll.run(12)
    end = _state5(b, tr)
    assert end["fit_steps"] >= mid["fit_steps"] + 3 and end["weights"] != mid["weights"]
    b.close()
    del b, tr, roll
    b, tr, roll = _build5(True)
    man = roll.restore(path)
    assert man["sections"]["replay_actor_values"]["shape"] == [2, M4, 2]
    assert man["trainer_fingerprint"]["actor_priorities"] is True
    after = _state5(b, tr)
    assert [k for k in after if after[k] != mid[k]] == []
    roll.run(12)
    got = _state5(b, tr)
    assert [k for k in got if got[k] != end[k]] == []
    b.close()
    del b, tr, roll
    # a checkpoint taken with the option off: no section, and refused under the option
    b, tr, roll = _build5(False)
    roll.run(6)
    roll.checkpoint(path_off)
    b.close()
    from ofighters_amd.checkpoint import Reader
    assert "replay_actor_values" not in Reader(path_off).sections
    b, tr, roll = _build5(True)
    with pytest.raises(ValueError, match="actor_priorities"):
        roll.restore(path_off)
    b.close()
