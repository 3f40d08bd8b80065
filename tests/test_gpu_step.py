"""GPU parity of the arena step (libofx.so through the C-ABI) against
 (1) the golden traces captured from the live reference, and
 (2) the CPU oracle on seeded random rollouts.
Bit-exact everywhere: ship coordinates / rewards / scores / kill indices are
integers; laser coordinates are accumulated doubles compared with ==.

Known measure-zero difference (documented in DESIGN.md): the reference
evaluates the laser-ship distance with libm pow() and the trajectory cone with
glibc atan2/atan; the GPU uses x*x and OCML.  A comparison could only flip for
inputs within ~1 ulp of a threshold; these tests report any such flip as a
failure (none is expected)."""
import numpy as np
import pytest

from tests.trace_util import load_trace, step_traces, trace_constants, unpack_map

pytestmark = pytest.mark.gpu

REP = 4  # replicate each trace in 4 arenas = one full 256-thread block


def _batch(n, m, **kw):
    from ofighters_amd import ArenaBatch
    return ArenaBatch(n, m, **kw)


@pytest.mark.parametrize("name", step_traces())
def test_step_trace_gpu(name):
    from ofighters_amd import pack_actions, _native as nat
    z = load_trace(name)
    M = z["init_state"].shape[0]
    ticks, episodes = int(z["ticks"]), int(z["episodes"])
    b = _batch(REP, M, laser_cap=256, **trace_constants(z))   # the step_const_* traces carry their own constants
    rep = lambda a: np.broadcast_to(a, (REP,) + a.shape)
    b.spawn(rep(z["spawn_draws"]))
    ini = z["init_state"]
    b.set_ships(x=rep(ini[:, 0]), y=rep(ini[:, 1]), px=rep(ini[:, 2]), py=rep(ini[:, 3]))
    sm, _ = b.maps_host(nat.MAP_U8)
    for r in range(REP):
        assert np.array_equal(sm[r], unpack_map(z["init_ship_map"]))
    map_idx = {int(t): k for k, t in enumerate(z["map_ticks"])}
    t = 0
    for ep in range(episodes):
        for _ in range(ticks):
            head, done = b.observe_head()
            assert np.array_equal(head, rep(z["obs8"][t])), (name, t, "obs head")
            assert np.array_equal(done, rep(z["obs_done"][t])), (name, t, "done")
            a = z["actions"][t]
            b.step(pack_actions(rep(a[:, 0]), rep(a[:, 1]), rep(a[:, 2]), rep(a[:, 3]), rep(a[:, 4])))
            assert np.array_equal(b.get(nat.F_OBS_REWARD), rep(z["obs8"][t][:, 0]).astype(np.int32))
            xy = np.stack([b.get(nat.F_SHIP_X), b.get(nat.F_SHIP_Y)], axis=-1)
            assert np.array_equal(xy, rep(z["ship_xy"][t])), (name, t, "ship xy")
            pt = np.stack([b.get(nat.F_SHIP_PX), b.get(nat.F_SHIP_PY)], axis=-1)
            assert np.array_equal(pt, rep(z["ship_pt"][t])), (name, t, "pointing")
            assert np.array_equal(b.get(nat.F_SHIP_ALIVE), rep(z["ship_alive"][t])), (name, t, "alive")
            assert np.array_equal(b.get(nat.F_REWARD), rep(z["reward"][t])), (name, t, "reward")
            assert np.array_equal(b.get(nat.F_SCORE), rep(z["score"][t])), (name, t, "score")
            n = int(z["n_lasers"][t])
            assert np.array_equal(b.get(nat.F_N_LASERS), np.full(REP, n)), (name, t, "n_lasers")
            lx, ly = b.get(nat.F_LASER_X)[:, :n], b.get(nat.F_LASER_Y)[:, :n]
            assert np.array_equal(lx, rep(z["laser_x"][t, :n])), (name, t, "laser x")
            assert np.array_equal(ly, rep(z["laser_y"][t, :n])), (name, t, "laser y")
            assert np.array_equal(b.get(nat.F_LASER_OWNER)[:, :n], rep(z["laser_owner"][t, :n])), (name, t, "owner")
            assert np.array_equal(b.get(nat.F_LASER_DEAD)[:, :n], rep(z["laser_destroyed"][t, :n])), (name, t, "dead")
            if t in map_idx:
                k = map_idx[t]
                sm, lm = b.maps_host(nat.MAP_U8)
                for r in range(REP):
                    assert np.array_equal(sm[r], unpack_map(z["ship_maps"][k])), (name, t, "ship map")
                    assert np.array_equal(lm[r], unpack_map(z["laser_maps"][k])), (name, t, "laser map")
                sb, lb = b.maps_host(nat.MAP_BITS)  # numpy.packbits-compatible output
                assert np.array_equal(sb[0], z["ship_maps"][k]) and np.array_equal(lb[0], z["laser_maps"][k])
            t += 1
        b.restart(rep(z["reset_draws"][ep]))
        xy = np.stack([b.get(nat.F_SHIP_X), b.get(nat.F_SHIP_Y), b.get(nat.F_SHIP_PX), b.get(nat.F_SHIP_PY)], axis=-1)
        assert np.array_equal(xy, rep(z["reset_state"][ep])), (name, ep, "reset")
        assert np.array_equal(b.get(nat.F_LAST_SCORES), rep(z["ep_scores"][ep])), (name, ep, "scores")
        assert np.all(b.get(nat.F_SHIP_ALIVE) == 1) and np.all(b.get(nat.F_SCORE) == 0)
        assert np.all(b.get(nat.F_N_LASERS) == 0)
        es = b.episode_scores_host()
        assert np.array_equal(es[:M], REP * z["ep_scores"][ep]) and es[M] == REP
    assert b.overflow_count() == 0
    b.close()


def _oracle_rollout(b, oracles, behaviours, seed, ticks, episode_ticks, arena_base=0, check_every=1, tick0=0):
    """Advance GPU batch and per-arena CPU oracles with the device bot law and
    compare the complete state: lock-steps tick0 .. tick0 + ticks - 1."""
    from ofighters_amd import _native as nat
    from oracle import pyoracle
    N, M = b.N, b.M
    beh = np.array([nat.BEHAVIOURS[x] for x in behaviours], dtype=np.int32)
    for t in range(tick0, tick0 + ticks):
        if t > 0 and t % episode_ticks == 0:
            b.restart_random(seed)
            for g, o in enumerate(oracles):
                o.restart(pyoracle.reset_draws(o.cfg, seed, arena_base + g, b.episode))
        b.bot_actions(behaviours, seed, tick=t)
        acts = b.actions_host()
        b.step(actions_ptr=b._actions.ptr)
        full = (t % check_every == 0) or t == tick0 + ticks - 1
        if full:
            X, Y, PX, PY = (b.get(f) for f in (nat.F_SHIP_X, nat.F_SHIP_Y, nat.F_SHIP_PX, nat.F_SHIP_PY))
            AL, RW, SC, KL = (b.get(f) for f in (nat.F_SHIP_ALIVE, nat.F_REWARD, nat.F_SCORE, nat.F_KILLER))
            NL, LX, LY, LO, LD = (b.get(f) for f in (nat.F_N_LASERS, nat.F_LASER_X, nat.F_LASER_Y,
                                                      nat.F_LASER_OWNER, nat.F_LASER_DEAD))
        for g, o in enumerate(oracles):
            want = o.bot_actions(beh, seed, arena_base + g, t)
            got = np.stack([acts[g]["valid"], acts[g]["shoot"], acts[g]["thrust"], acts[g]["px"], acts[g]["py"]],
                           axis=1).astype(np.int32)
            assert np.array_equal(got, want), (g, t, "bot actions")
            o.step(want)
            if not full:
                continue
            s = o.ships()
            assert np.array_equal(np.stack([X[g], Y[g]], 1), s["xy"]), (g, t, "xy")
            assert np.array_equal(np.stack([PX[g], PY[g]], 1), s["pt"]), (g, t, "pointing")
            assert np.array_equal(AL[g], s["alive"]), (g, t, "alive")
            assert np.array_equal(RW[g], s["reward"]), (g, t, "reward")
            assert np.array_equal(SC[g], s["score"]), (g, t, "score")
            assert np.array_equal(KL[g], s["killer"]), (g, t, "killer index")
            l = o.lasers()
            n = len(l["x"])
            assert NL[g] == n, (g, t, "n_lasers", NL[g], n)
            assert np.array_equal(LX[g, :n], l["x"]) and np.array_equal(LY[g, :n], l["y"]), (g, t, "laser xy")
            assert np.array_equal(LO[g, :n], l["owner"]) and np.array_equal(LD[g, :n], l["destroyed"]), (g, t, "laser meta")


def _spawn_both(b, seed, arena_base=0):
    from oracle import pyoracle
    b.spawn_random(seed)
    oracles = []
    for g in range(b.N):
        o = pyoracle.Arena(n_ships=b.M)
        o.spawn(pyoracle.reset_draws(o.cfg, seed, arena_base + g, 0))
        oracles.append(o)
    return oracles


@pytest.mark.parametrize("M,behaviours", [
    (8, ["random"] * 8),
    (4, ["random"] * 4),
    (8, ["turret", "turret", "runner", "random", "shoot", "thrust", "idle", "turret"]),
    (13, ["random"] * 7 + ["turret"] * 6),           # M not a power of two: pair windows straddle lanes
])
def test_random_rollout_vs_oracle(M, behaviours):
    b = _batch(128, M, laser_cap=512)
    oracles = _spawn_both(b, seed=0x0F160001)
    _oracle_rollout(b, oracles, behaviours, 0x0F160001, ticks=450, episode_ticks=200)
    assert b.overflow_count() == 0
    b.close()


def test_dense_brawl_vs_oracle():
    """Small map => constant close-quarters contact: kills, multi-kills, self
    hits, aim/trajectory rewards and border clamps every few ticks."""
    b = _batch(256, 8, laser_cap=256, width=64, height=64)
    from oracle import pyoracle
    b.spawn_random(5)
    oracles = []
    for g in range(b.N):
        o = pyoracle.Arena(cfg=pyoracle.default_cfg(8, width=64, height=64))
        o.spawn(pyoracle.reset_draws(o.cfg, 5, g, 0))
        oracles.append(o)
    _oracle_rollout(b, oracles, ["turret"] * 4 + ["random"] * 4, 5, ticks=240, episode_ticks=20)
    assert int((b.get(__import__("ofighters_amd")._native.F_SHIP_ALIVE) == 0).sum()) > 0
    b.close()


def test_laser_capacity_overflow_is_counted():
    """64 slots, 8 turrets firing 80% of ticks on a big map: the list fills up;
    dropped lasers are counted, never silently truncated, state stays sane."""
    from ofighters_amd import _native as nat
    b = _batch(8, 8, laser_cap=64)
    b.spawn_random(3)
    for t in range(60):
        b.bot_actions(["turret"] * 8, 3, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    assert np.all(b.get(nat.F_N_LASERS) <= 64)
    assert b.overflow_count() > 0
    assert b.overflow_count() == 0  # reading resets the counter
    b.close()


def test_sharding_invariance_and_determinism():
    """Arenas are keyed by GLOBAL id: two half batches with arena_base 0 / 64
    reproduce one 128-arena batch bit for bit; re-running reproduces itself."""
    from ofighters_amd import _native as nat

    def run(n, base):
        b = _batch(n, 8, arena_base=base)
        b.spawn_random(11)
        for t in range(230):
            if t == 200:
                b.restart_random(11)
            b.bot_actions(["random"] * 8, 11, tick=t)
            b.step(actions_ptr=b._actions.ptr)
        out = [b.get(f).copy() for f in (nat.F_SHIP_X, nat.F_SHIP_Y, nat.F_SCORE, nat.F_REWARD, nat.F_N_LASERS,
                                         nat.F_LASER_X, nat.F_LAST_SCORES)]
        es = b.episode_scores_host()
        b.close()
        return out, es

    full, es_full = run(128, 0)
    again, _ = run(128, 0)
    lo, es_lo = run(64, 0)
    hi, es_hi = run(64, 64)
    for a, c in zip(full, again):
        assert np.array_equal(a, c)
    for a, l, h in zip(full, lo, hi):
        assert np.array_equal(a, np.concatenate([l, h], axis=0))
    assert np.array_equal(es_full, es_lo + es_hi)  # what the RCCL all-reduce sums


@pytest.mark.parametrize("observe", [False, True])
def test_rollout_k_ticks_equal_single_ticks(observe):
    """ofx_rollout (the headless loop, battleground.py:169-173): K lock-steps of bots + step [+ rasterise] enqueued by
    one host call - without an observer all K inside ONE kernel launch - leave exactly the state bits of K single
    (ofx_bot_actions, ofx_step[, ofx_rasterise]) calls; also across an episode end and through ShardedRollout."""
    from ofighters_amd import _native as nat
    from ofighters_amd.rollout import ShardedRollout
    beh = ["random", "turret", "runner", "shoot", "thrust", "idle", "random", "turret"]
    fields = (nat.F_SHIP_X, nat.F_SHIP_Y, nat.F_SHIP_PX, nat.F_SHIP_PY, nat.F_SHIP_ALIVE, nat.F_REWARD, nat.F_SCORE,
              nat.F_OBS_REWARD, nat.F_KILLER, nat.F_HULL, nat.F_N_LASERS, nat.F_LASER_X, nat.F_LASER_Y, nat.F_LASER_DX,
              nat.F_LASER_DY, nat.F_LASER_OWNER, nat.F_LASER_DEAD, nat.F_TIME, nat.F_LAST_SCORES)
    N, seed = 300, 77                         # not a multiple of 4: the last block has idle waves
    one = _batch(N, 8, arena_base=17, laser_cap=128)
    many = _batch(N, 8, arena_base=17, laser_cap=128)
    one.spawn_random(seed)
    many.spawn_random(seed)
    mt = nat.MAP_U8 if observe else None
    t = 0
    for n in (1, 63, 96):                     # 160 lock-steps, the episode ends at 160
        for k in range(n):
            one.bot_actions(beh, seed, tick=t + k)
            one.step()
            if observe:
                one.rasterise()
        many.rollout(beh, seed, t, n, mt)
        t += n
        for f in fields:
            assert np.array_equal(one.get(f), many.get(f)), (n, f)
    if observe:
        for a, c in zip(one.maps_host(nat.MAP_U8), many.maps_host(nat.MAP_U8)):
            assert np.array_equal(a, c)
    assert one.overflow_count() == many.overflow_count()
    one.close(); many.close()
    # the same through the rollout driver: per-tick calls against the K-tick fast path, two episode ends inside
    logs = []
    for fast in (False, True):
        b = _batch(N, 8, arena_base=17)
        r = ShardedRollout(b, beh, seed, episode_ticks=50, observe=observe, use_rollout=fast)
        r.run(30); r.run(95)
        logs.append(([b.get(f).copy() for f in fields], [s.copy() for s in r.score_log]))
        b.close()
    assert len(logs[0][1]) == 2
    for a, c in zip(logs[0][0], logs[1][0]):
        assert np.array_equal(a, c)
    for a, c in zip(logs[0][1], logs[1][1]):
        assert np.array_equal(a, c)


def test_lock_step_forms_agree_on_a_non_square_map():
    """The three forms of the lock-step - single (ofx_bot_actions, ofx_step) calls, ofx_rollout and ofx_step_repeat
    with nobody holding - on a 96 x 64 map: a swap of W and H in the bots' repoint draw or in the reset draw is
    invisible on a square one.  5 arenas (the last block has idle waves), 13 ships on all six laws, 40 lock-steps as
    1 + 7 + 32 with an episode end (restart_random) after the eighth; the single calls are held to the CPU oracle
    lock-step by lock-step, the other two to the single calls, every field with ==."""
    from ofighters_amd import _native as nat
    from oracle import pyoracle
    N, M, W, H, seed, base = 5, 13, 96, 64, 4242, 3
    beh = (["random", "turret", "runner", "shoot", "thrust", "idle"] * 3)[:M]
    assert {nat.BEHAVIOURS[x] for x in beh} == set(nat.BEHAVIOURS.values())
    fields = (nat.F_SHIP_X, nat.F_SHIP_Y, nat.F_SHIP_PX, nat.F_SHIP_PY, nat.F_SHIP_ALIVE, nat.F_REWARD, nat.F_SCORE,
              nat.F_OBS_REWARD, nat.F_KILLER, nat.F_HULL, nat.F_N_LASERS, nat.F_LASER_X, nat.F_LASER_Y, nat.F_LASER_DX,
              nat.F_LASER_DY, nat.F_LASER_OWNER, nat.F_LASER_DEAD, nat.F_TIME, nat.F_LAST_SCORES)
    single, roll, rep = (_batch(N, M, laser_cap=64, width=W, height=H, arena_base=base) for _ in range(3))
    oracles = []
    for g in range(N):
        o = pyoracle.Arena(cfg=pyoracle.default_cfg(M, width=W, height=H))
        o.spawn(pyoracle.reset_draws(o.cfg, seed, base + g, 0))
        oracles.append(o)
    for b in (single, roll, rep):
        b.spawn_random(seed)
    t = 0
    for n in (1, 7, 32):
        if t == 8:
            for b in (single, roll, rep):
                b.restart_random(seed)
            for g, o in enumerate(oracles):
                o.restart(pyoracle.reset_draws(o.cfg, seed, base + g, single.episode))
        _oracle_rollout(single, oracles, beh, seed, ticks=n, episode_ticks=10 ** 9, arena_base=base, tick0=t)
        roll.rollout(beh, seed, t, n)
        rep.step_repeat(beh, seed, t, n)
        t += n
        for f in fields:
            want = single.get(f)
            assert np.array_equal(roll.get(f), want), (n, f, "rollout")
            assert np.array_equal(rep.get(f), want), (n, f, "step_repeat")
    assert single.episode == 1 and (single.get(nat.F_TIME) == 32).all()
    assert int((single.get(nat.F_SHIP_ALIVE) == 0).sum()) > 0 and int(single.get(nat.F_N_LASERS).sum()) > 0
    for b in (single, roll, rep):
        assert b.overflow_count() == 0      # the oracle's laser list has no capacity
        b.close()


def test_full_size_properties():
    """BASELINE config 2 size (4096 x 8): size-independent properties + a
    random sample of arenas replayed on the oracle."""
    from ofighters_amd import _native as nat
    from oracle import pyoracle
    N, M, seed = 4096, 8, 0x0F160001
    b = _batch(N, M)
    b.spawn_random(seed)
    rs = np.random.RandomState(0)
    sample = np.sort(rs.choice(N, 48, replace=False))
    oracles = {}
    for g in sample:
        o = pyoracle.Arena(n_ships=M)
        o.spawn(pyoracle.reset_draws(o.cfg, seed, int(g), 0))
        oracles[int(g)] = o
    beh = np.full(M, nat.BOT_RANDOM, np.int32)
    prev_alive = b.get(nat.F_SHIP_ALIVE).copy()
    score_bank = np.zeros((N, M), np.int64)
    for t in range(420):
        if t > 0 and t % 200 == 0:
            sc_before = b.get(nat.F_SCORE).astype(np.int64)
            b.restart_random(seed)
            es = b.episode_scores_host()
            assert np.array_equal(es[:M], sc_before.sum(0)) and es[M] == N   # checksum of checksums
            assert np.array_equal(b.get(nat.F_LAST_SCORES), sc_before)
            for g, o in oracles.items():
                o.restart(pyoracle.reset_draws(o.cfg, seed, g, b.episode))
            prev_alive = b.get(nat.F_SHIP_ALIVE).copy()
            assert prev_alive.all()
        b.bot_actions(["random"] * M, seed, tick=t)
        acts = b.actions_host()
        rew_before = b.get(nat.F_REWARD).astype(np.int64)
        sc_before = b.get(nat.F_SCORE).astype(np.int64)
        b.step(actions_ptr=b._actions.ptr)
        # Agent.step bookkeeping: score += reward happens for every ship, dead included
        assert np.array_equal(b.get(nat.F_SCORE), sc_before + rew_before)
        alive = b.get(nat.F_SHIP_ALIVE)
        assert not np.any(alive & ~prev_alive.astype(bool))               # no resurrection inside an episode
        killer = b.get(nat.F_KILLER)
        assert np.array_equal(killer >= 0, (prev_alive == 1) & (alive == 0))  # died this tick <=> has a killer
        nl = b.get(nat.F_N_LASERS)
        assert nl.min() >= 0 and nl.max() <= b.L
        x, y = b.get(nat.F_SHIP_X), b.get(nat.F_SHIP_Y)
        assert x.min() >= 0 and y.min() >= 0 and x.max() <= 400 and y.max() <= 400
        prev_alive = alive.copy()
        for g, o in oracles.items():
            a = acts[g]
            o.step(np.stack([a["valid"], a["shoot"], a["thrust"], a["px"], a["py"]], axis=1).astype(np.int32))
        if t % 20 == 19:
            LX, LY = b.get(nat.F_LASER_X), b.get(nat.F_LASER_Y)
            RW = b.get(nat.F_REWARD)
            for g, o in oracles.items():
                s, l = o.ships(), o.lasers()
                n = len(l["x"])
                assert nl[g] == n
                assert np.array_equal(LX[g, :n], l["x"]) and np.array_equal(LY[g, :n], l["y"])
                assert np.array_equal(np.stack([x[g], y[g]], 1), s["xy"])
                assert np.array_equal(alive[g], s["alive"]) and np.array_equal(RW[g], s["reward"])
    assert b.overflow_count() == 0
    b.close()


def test_error_behaviour():
    from ofighters_amd import OfxError, _native as nat
    b = _batch(4, 4)
    with pytest.raises(OfxError):            # step before spawn
        b.step(actions_ptr=b._actions.ptr)
    with pytest.raises(OfxError, match="before ofx_spawn"):
        b.rollout(["idle"] * 4, 1, 0, 5)
    b.spawn_random(1)
    t_before = b.get(nat.F_TIME).copy()
    b.rollout(["idle"] * 4, 1, 0, 0)         # zero lock-steps: a no-op
    assert np.array_equal(b.get(nat.F_TIME), t_before)
    with pytest.raises(OfxError, match="observe_map_type"):
        b.rollout(["idle"] * 4, 1, 0, 3, observe=7)
    with pytest.raises(Exception):           # agents/agent.py:51, before any lock-step runs
        b.rollout(["idle", "kamikaze", "idle", "idle"], 1, 0, 3)
    assert np.array_equal(b.get(nat.F_TIME), t_before)
    b.close()
    b = _batch(4, 4)
    with pytest.raises(Exception):           # agents/agent.py:51
        b.spawn_random(1)
        b.bot_actions(["kamikaze"] * 4, 1)
    b.close()


@pytest.mark.parametrize("M,W,H,L", [(1, 400, 400, 64), (64, 96, 96, 1024), (5, 64, 128, 256), (7, 160, 96, 256)])
def test_shapes_and_non_square_maps_vs_oracle(M, W, H, L):
    """Edge shapes: a lone ship, a full wave of 64 ships (4096 shooter/enemy pairs), and NON-SQUARE arenas where the
    reference's map is np.zeros((dim.x, dim.y)) indexed [y][x] (observation.py:86, form.py:226): the quirk
    (rows bounded by the width) is reproduced, not fixed."""
    from ofighters_amd import _native as nat
    from oracle import pyoracle
    N, seed = 16, 1234 + M
    b = _batch(N, M, laser_cap=L, width=W, height=H)
    b.spawn_random(seed)
    oracles = []
    for g in range(N):
        o = pyoracle.Arena(cfg=pyoracle.default_cfg(M, width=W, height=H))
        o.spawn(pyoracle.reset_draws(o.cfg, seed, g, 0))
        oracles.append(o)
    beh = (["turret", "random", "runner", "shoot", "thrust", "idle"] * 11)[:M]
    _oracle_rollout(b, oracles, beh, seed, ticks=90, episode_ticks=40, check_every=3)
    sm, lm = b.maps_host(nat.MAP_U8)
    assert sm.shape == (N, W, H)
    for g, o in enumerate(oracles):
        osm, olm = o.rasterise()
        assert np.array_equal(sm[g], osm) and np.array_equal(lm[g], olm), g
    assert b.overflow_count() == 0
    b.close()
