"""Per-arena episodes on the device: ofx_restart_finished against the global restart it generalises and against the CPU
model (tests/autoreset_oracle.py) lock-step by lock-step, its groups, the `seen` latches and the replay memory, its
argument errors and state round trip, and TrainingRollout(auto_reset=True) end to end and through a checkpoint.
Every comparison is `==`."""
import ctypes as C

import numpy as np
import pytest

from tests import autoreset_oracle as ao
from tests import repeat_oracle as ro

pytestmark = pytest.mark.gpu

N = ao.N
SHIP_FIELDS = ("F_SHIP_X", "F_SHIP_Y", "F_SHIP_PX", "F_SHIP_PY", "F_SHIP_ALIVE", "F_HULL", "F_REWARD", "F_OBS_REWARD",
               "F_SCORE", "F_KILLER", "F_LAST_SCORES", "F_TIME")
LASER_FIELDS = ("F_LASER_X", "F_LASER_Y", "F_LASER_DX", "F_LASER_DY", "F_LASER_OWNER", "F_LASER_DEAD")


def _batch(m, seed, **cfg):
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, m, **dict(ro.REWARDS, **cfg))
    b.spawn_random(seed)
    return b


def _state(b):
    """Every ship field, the clock, n_lasers and the live prefix of all laser arrays."""
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


def _against_model(st, snap):
    """The names of what differs between a device state (_state) and a model snapshot."""
    bad = []
    for g in range(N):
        o, l = snap["ships"][g], snap["lasers"][g]
        pairs = [("xy", np.stack([st["F_SHIP_X"][g], st["F_SHIP_Y"][g]], 1), o["xy"]),
                 ("pt", np.stack([st["F_SHIP_PX"][g], st["F_SHIP_PY"][g]], 1), o["pt"]),
                 ("n_lasers", st["n_lasers"][g], len(l["x"])),
                 ("laser_x", st["F_LASER_X"][g], l["x"]), ("laser_y", st["F_LASER_Y"][g], l["y"]),
                 ("laser_owner", st["F_LASER_OWNER"][g], l["owner"]), ("laser_dead", st["F_LASER_DEAD"][g], l["destroyed"])]
        pairs += [(key, st[f][g], o[key]) for f, key in (("F_SHIP_ALIVE", "alive"), ("F_REWARD", "reward"),
                                                         ("F_SCORE", "score"), ("F_KILLER", "killer"), ("F_HULL", "hull"),
                                                         ("F_LAST_SCORES", "last_score"))]
        bad += ["%s[%d]" % (name, g) for name, got, want in pairs if not np.array_equal(got, want)]
    if not np.array_equal(st["F_TIME"], snap["time"]):
        bad.append("time")
    return bad


class _Auto:
    """The device side of one restart_finished caller: the ship mask, the sums and optionally groups and `seen`."""

    def __init__(self, b, selected, group=None, n_groups=1, seen=False):
        from ofighters_amd import DeviceBuffer
        self.b, self.G = b, n_groups
        self.mask = None
        if selected is not None:
            mk = np.zeros((b.N, b.M), np.uint8)
            mk[:, list(selected)] = 1
            self.mask = DeviceBuffer(mk.nbytes).upload(mk)
        self.sums = DeviceBuffer(8 * n_groups * (b.M + 2)).upload(np.zeros((n_groups, b.M + 2), np.int64))
        self.group = None if group is None else DeviceBuffer(4 * b.N).upload(np.asarray(group, np.int32))
        self.seen = DeviceBuffer(b.N * b.M).upload(np.ones((b.N, b.M), np.uint8)) if seen else None

    def call(self, seed, max_ticks):
        self.b.restart_finished(seed, self.mask.ptr if self.mask else None, max_ticks, self.seen, self.group, self.G,
                                self.sums)

    def sums_host(self):
        self.b.sync()
        return self.sums.download(np.int64, (self.G, self.b.M + 2))


# ------------------------------------------------------------------------- a. nobody dies: the global restart, bit for bit
def test_zero_mask_is_the_global_restart():
    m, seed, ticks = 8, 777, 10
    beh = ao.behaviours(m)
    a, b = _batch(m, seed), _batch(m, seed)                      # a: restart_finished, b: restart_random every 10th
    au = _Auto(a, ())
    running = np.zeros(m + 1, np.int64)
    for t in range(35):
        au.call(seed, ticks)
        if t and t % ticks == 0:
            b.restart_random(seed)
            running += b.episode_scores()
        for x in (a, b):
            x.bot_actions(beh, seed, tick=t)
            x.step()
        assert _differences(_state(a), _state(b)) == [], t
        s = au.sums_host()
        assert np.array_equal(s[0, :m + 1], running), t
        assert s[0, m + 1] == s[0, m] * ticks, t
        st = a.autoreset_state()
        assert (st["arena_episode"] == b.episode).all() and not st["dead_once"].any()
        assert (st["restarted"] == (1 if t and t % ticks == 0 else 0)).all()
    assert b.episode == 3 and running[m] == 3 * N and running[:m].any()
    assert (a.episode_scores() == 0).all()                       # ofx_episode_scores' sums are not touched
    a.close(), b.close()


def test_zero_mask_is_the_global_restart_on_a_non_square_map():
    """The same scenario at 5 arenas x 3 ships on 96 x 64, where a swap of W and H in restart_finished's reset draw
    would show: == the global restart lock-step by lock-step, and the restarted ships stand where
    pyoracle.reset_draws puts them in episode 1 (a draw of 0 keeps the coordinate: ship.py:100-101)."""
    from ofighters_amd import ArenaBatch, _native as nat
    from oracle import pyoracle
    n, m, w, h, seed, ticks = 5, 3, 96, 64, 779, 10
    beh = ao.behaviours(m)
    a, b = (ArenaBatch(n, m, **dict(ro.REWARDS, width=w, height=h, laser_cap=64)) for _ in range(2))
    for x in (a, b):
        x.spawn_random(seed)
    au = _Auto(a, ())
    for t in range(ticks + 3):
        old = np.stack([a.get(nat.F_SHIP_X), a.get(nat.F_SHIP_Y)], 2)
        au.call(seed, ticks)
        if t == ticks:
            b.restart_random(seed)
            cfg = pyoracle.default_cfg(m, width=w, height=h)
            draws = np.stack([pyoracle.reset_draws(cfg, seed, g, 1) for g in range(n)])
            assert draws[..., 0].max() > h                        # an x draw no y draw can give
            now = np.stack([a.get(nat.F_SHIP_X), a.get(nat.F_SHIP_Y)], 2)
            assert np.array_equal(now, np.where(draws != 0, draws, old))
        assert _differences(_state(a), _state(b)) == [], t
        st = a.autoreset_state()
        assert (st["arena_episode"] == b.episode).all() and (st["restarted"] == (1 if t == ticks else 0)).all()
        for x in (a, b):
            x.bot_actions(beh, seed, tick=t)
            x.step()
    assert b.episode == 1
    a.close(), b.close()


# ------------------------------------------------------------------------------------------ b. the scenarios of the model
CASES = {
    "M8": dict(ao.SCENARIOS["M8"]),
    "M13": dict(ao.SCENARIOS["M13"]),
    "base7": dict(ao.SCENARIOS["M8"], arena_base=7),             # the counter's key is the GLOBAL arena
    "null_mask": dict(ao.SCENARIOS["M8"], selected=None),        # NULL selects every ship
}


def _run_against_model(kw, group=None, n_groups=1):
    sc = ao.run(group=group, n_groups=n_groups, **kw)
    b = _batch(kw["m"], kw["seed"], arena_base=kw.get("arena_base", 0))
    au = _Auto(b, kw["selected"], group, n_groups)
    beh = ao.behaviours(kw["m"])
    for t in range(ao.STEPS):
        au.call(kw["seed"], ao.MAX_TICKS)
        b.bot_actions(beh, kw["seed"], tick=t)
        b.step()
        snap = sc["snapshots"][t]
        assert _against_model(_state(b), snap) == [], t
        st = b.autoreset_state()
        assert np.array_equal(st["arena_episode"], snap["arena_episode"]), t
        assert np.array_equal(st["dead_once"], snap["dead_once"]), t
        assert np.array_equal(st["restarted"], snap["restarted"]) and np.array_equal(st["restarted"], sc["restarts"][t]), t
        assert np.array_equal(au.sums_host(), snap["sums"]), t
    assert b.overflow_count() == 0
    final = au.sums_host()
    b.close()
    return sc, final


@pytest.mark.parametrize("case", list(CASES))
def test_scenario_against_the_model(case):
    sc, sums = _run_against_model(CASES[case])
    assert sc["restarts"].sum() >= 10 and sums[0, -2] == sc["restarts"].sum()
    if case != "null_mask":
        assert sc["by_death"] >= 1 and sc["by_clock"] >= 1


# ----------------------------------------------------------------------------------------------------------- c. groups
def test_groups():
    kw = ao.SCENARIOS["M8"]
    group = [0, 1, -1, 0, 1]
    sc, grouped = _run_against_model(kw, group=group, n_groups=2)
    assert grouped[:, -2].min() >= 1                             # both groups finished episodes
    ungrouped = ao.run(**kw)["snapshots"][-1]["sums"]            # pinned to the device by the case "M8" above
    left_out = ao.run(group=[-1, -1, 0, -1, -1], n_groups=1, **kw)["snapshots"][-1]["sums"]
    assert left_out[0, -2] >= 1
    assert np.array_equal(grouped.sum(axis=0) + left_out[0], ungrouped[0])
    # a group value outside [0, n_groups) counts nowhere, like -1; the arenas restart all the same
    b = _batch(kw["m"], kw["seed"])
    au = _Auto(b, kw["selected"], [0, 1, 2, 0, 1], 2)
    beh = ao.behaviours(kw["m"])
    for t in range(ao.STEPS):
        au.call(kw["seed"], ao.MAX_TICKS)
        b.bot_actions(beh, kw["seed"], tick=t)
        b.step()
    assert np.array_equal(au.sums_host(), grouped)
    assert np.array_equal(b.autoreset_state()["arena_episode"], sc["episodes"])
    b.close()


# ---------------------------------------------------------------------------------- d. `seen` and the replay memory
def _rows_equal(dev, ora):
    assert len(dev) == len(ora), (len(dev), len(ora))
    for d, o in zip(dev, ora):
        assert (d["tick_prev"], d["tick_next"], d["ship"], d["iaction"], d["px"], d["py"], d["reward"], d["done"]) == \
               tuple(int(v) for v in o[:8]), (d, o)
        assert np.array_equal(d["head_prev"], o[8]) and np.array_equal(d["head_next"], o[9])


@pytest.mark.parametrize("packed", [False, True])
def test_seen_and_the_replay_memory(packed):
    """The one-ship mask: every death of ship 0 ends its arena's episode.  A capture per lock-step, after the call."""
    from oracle import pyoracle
    kw = dict(seed=777, m=8, selected=(0,))
    sc = ao.run(**kw)
    assert sc["by_death"] >= 3 and sc["by_clock"] >= 1
    cap = 128                                                    # >= the lock-steps: no row is overwritten
    b = _batch(kw["m"], kw["seed"])
    b.replay_create(cap, 0, packed=packed)
    au = _Auto(b, kw["selected"], seen=True)
    mems = [pyoracle.ReplayMemory(kw["m"], cap) for _ in range(N)]
    beh = ao.behaviours(kw["m"])
    want_seen = np.ones((N, kw["m"]), np.uint8)
    for t in range(ao.STEPS):
        au.call(kw["seed"], ao.MAX_TICKS)
        b.sync()
        want_seen[sc["restarts"][t] != 0] = 0                    # only the restarted arenas are cleared
        assert np.array_equal(au.seen.download(np.uint8, (N, kw["m"])), want_seen), t
        b.replay_capture(t, au.mask.ptr)                         # the handle's (iaction, ipointer): zeros
        for g in range(N):
            if sc["restarts"][t][g]:
                mems[g].reset()
            mems[g].play(t, 0, sc["heads"][t][g, 0], bool(sc["dones"][t][g, 0]), (0, (0, 0)))
        b.bot_actions(beh, kw["seed"], tick=t)
        b.step()
    cnt, app = b.replay_count()
    for g in range(N):
        rows = b.replay_rows(g)
        assert cnt[g] == len(mems[g].rows()) and app[g] == mems[g].appended
        _rows_equal(rows, mems[g].rows())
        assert all(r["tick_next"] - r["tick_prev"] == 1 and r["ship"] == 0 for r in rows)
        starts = [0] + [int(t) for t in np.flatnonzero(sc["restarts"][:, g])]
        for t in np.flatnonzero(sc["deaths"][:, g]):
            t, begun = int(t), max(s for s in starts if s < t)
            ended = [r for r in rows if begun < r["tick_next"] < t and r["done"]]
            # one losing frame per episode, captured on the lock-step between the two calls that saw the ship dead
            assert len(ended) == 1 and ended[0]["tick_next"] == t - 1, (g, t)
            assert not any(r["tick_prev"] < t <= r["tick_next"] for r in rows), (g, t)      # no row spans a restart
            if t + 2 < ao.STEPS:
                assert any(r["tick_prev"] == t for r in rows), (g, t)                       # rows appear again
    assert sum(int(r["done"]) for g in range(N) for r in b.replay_rows(g)) >= sc["by_death"]
    b.close()


# ------------------------------------------------------------------------ e. argument errors and the state round trip
def test_errors_and_state_round_trip():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    L = nat.lib()
    m = 8
    b = ArenaBatch(N, m)
    sums = DeviceBuffer(8 * (m + 2)).upload(np.zeros(m + 2, np.int64))
    group = DeviceBuffer(4 * N).upload(np.zeros(N, np.int32))
    call = lambda h, max_ticks=0, group=None, n_groups=1, sums=None: L.ofx_restart_finished(h, 1, None, max_ticks, None,
                                                                                            group, n_groups, sums)
    assert call(b.handle) == nat.OFX_ERR_STATE                   # before a spawn
    ep = np.zeros(N, np.uint32)
    assert L.ofx_autoreset_set_state(b.handle, ep.ctypes.data_as(C.c_void_p), None) == nat.OFX_ERR_STATE
    b.spawn_random(1)
    with pytest.raises(OfxError) as err:
        b.autoreset_state()                                      # nothing allocated yet
    assert err.value.code == nat.OFX_ERR_STATE
    assert call(None) == nat.OFX_ERR_INVALID
    assert call(b.handle, max_ticks=-1) == nat.OFX_ERR_INVALID
    assert call(b.handle, n_groups=0, sums=sums.ptr) == nat.OFX_ERR_INVALID
    assert call(b.handle, n_groups=N + 1, sums=sums.ptr) == nat.OFX_ERR_INVALID
    assert call(b.handle, group=group.ptr) == nat.OFX_ERR_INVALID
    assert L.ofx_autoreset_state_host(None, None, None, None) == nat.OFX_ERR_INVALID
    assert L.ofx_autoreset_set_state(None, None, None) == nat.OFX_ERR_INVALID
    with pytest.raises(OfxError):
        b.autoreset_state()                                      # a refused call allocates nothing
    assert call(b.handle, group=group.ptr, n_groups=N, sums=sums.ptr) == nat.OFX_OK
    st = b.autoreset_state()
    assert st["arena_episode"].dtype == np.uint32 and st["dead_once"].shape == (N, m) and st["restarted"].shape == (N,)
    assert not st["arena_episode"].any() and not st["dead_once"].any() and not st["restarted"].any()
    # set_state + readback is the identity
    rs = np.random.RandomState(5)
    want = {"arena_episode": rs.randint(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32),
            "dead_once": rs.randint(0, 2, (N, m)).astype(np.uint8)}
    b.load_autoreset_state(want)
    st = b.autoreset_state()
    assert np.array_equal(st["arena_episode"], want["arena_episode"]) and np.array_equal(st["dead_once"], want["dead_once"])
    for bad in (dict(want, arena_episode=want["arena_episode"].astype(np.int64)), dict(want, dead_once=want["dead_once"][:-1]),
                {"arena_episode": want["arena_episode"]}):
        with pytest.raises(ValueError):
            b.load_autoreset_state(bad)
    # ofx_restart clears dead_once of the arenas it restarts and leaves arena_episode alone; a spawn zeroes both
    want["dead_once"][:] = 1
    b.load_autoreset_state(want)
    amask = np.array([1, 0, 0, 1, 0], np.uint8)
    b.restart(np.zeros((N, m, 2), np.int32), amask)
    st = b.autoreset_state()
    assert np.array_equal(st["dead_once"], np.repeat(1 - amask, m).reshape(N, m))
    assert np.array_equal(st["arena_episode"], want["arena_episode"])
    b.restart_random(1)
    st = b.autoreset_state()
    assert not st["dead_once"].any() and np.array_equal(st["arena_episode"], want["arena_episode"])
    b.load_autoreset_state(want)
    b.spawn_random(1)
    st = b.autoreset_state()
    assert not st["dead_once"].any() and not st["arena_episode"].any()
    assert set(b.state_dict()) == set(ArenaBatch.STATE_FIELDS) | {"episode", "tick"}      # the key set stays
    b.close()


# ------------------------------------------------------------------------------------- f. TrainingRollout(auto_reset=True)
RN, RSEED, TICKS = 6, 3, 20      # seed 3: on the CPU model (ship 0 on the random bot's law, the others as here) the 6 arenas
                                 # append 336 rows in 60 lock-steps with per-arena episodes and 299 without (10 deaths)


def _build(auto_reset=True, **roll_kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(RN, ro.M, **ro.REWARDS)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=64, fit_batch=8)
    roll = TrainingRollout(b, tr, ro.BEHAVIOURS, RSEED, policy_ships=(0,), episode_ticks=TICKS, collecting_steps=3,
                           replay_every=2, auto_reset=auto_reset, **roll_kw)
    return b, tr, roll


def _train_state(b, tr, roll):
    b.sync()
    s = {"weights": tr.weights_host().tobytes(), "adam_m": tr.adam_m.download(np.float32, (tr.n_floats,)).tobytes(),
         "adam_v": tr.adam_v.download(np.float32, (tr.n_floats,)).tobytes(), "losses": list(tr.losses),
         "roll_losses": list(roll.losses), "fit_steps": tr.fit_steps, "epsilon": tr.epsilon.get(),
         "counters": (roll.tick, roll.total_steps, roll.capture_tick, roll.episode, b.episode, b.tick),
         "rows": [b.replay_rows(g).tobytes() for g in range(RN)],
         "count": [x.tobytes() for x in b.replay_count()],
         "seen": roll._seen_done.download(np.uint8, (RN, ro.M)).tobytes(),
         "score_log": [x.tobytes() for x in roll.score_log], "length_log": [x.tobytes() for x in roll.length_log],
         "epsilons": list(roll.epsilons)}
    if roll.auto_reset:
        st = b.autoreset_state()
        s["arena_episode"], s["dead_once"] = st["arena_episode"].tobytes(), st["dead_once"].tobytes()
        s["sums"] = roll._auto_sums.download(np.int64, (1, ro.M + 2)).tobytes()
    for f in range(19):
        s["field%d" % f] = b.get(f).tobytes()
    return s


@pytest.mark.parametrize("K", [1, 2])
def test_training_rollout_auto_reset(tmp_path, K):
    """60 lock-steps (K = 2: 20 decisions): two runs from scratch are bit-identical, and a checkpoint half way,
    restored into fresh handles, continues equal to the uninterrupted run."""
    kw = dict(action_repeat=K) if K > 1 else {}
    half = 30 if K == 1 else 10
    b, tr, roll = _build(**kw)
    roll.run(half)
    mid = _train_state(b, tr, roll)
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    roll.run(half)
    end = _train_state(b, tr, roll)
    appended_on = int(b.replay_count()[1].sum())
    episodes = b.autoreset_state()["arena_episode"]
    # (the period that ends with the last lock-step is reported at the head of the next one)
    assert b.episode == 0 and roll.episode == (2 * half * K - 1) // TICKS and len(roll.length_log) == roll.episode
    assert end["fit_steps"] >= mid["fit_steps"] + 3 and np.isfinite(roll.losses).all()
    # an arena restarts at least with the clock; every finished episode is in a reporting period or in the running sums
    assert (episodes >= roll.episode).all()
    if K == 1:
        assert episodes.max() > roll.episode                     # ... and some arena because its learner died
    sums = roll._auto_sums.download(np.int64, (1, ro.M + 2))
    assert sum(int(x[ro.M]) for x in roll.score_log) + sums[0, ro.M] == episodes.sum()
    assert sum(int(x[0]) for x in roll.length_log) + sums[0, ro.M + 1] + b.get(13).sum() == RN * 2 * half * K
    for g in range(RN):
        assert all(r["tick_next"] - r["tick_prev"] == 1 for r in b.replay_rows(g))
    b.close()
    del b, tr, roll

    b, tr, roll = _build(**kw)                                   # the same run again, uninterrupted
    roll.run(2 * half)
    again = _train_state(b, tr, roll)
    assert [k for k in again if again[k] != end[k]] == []
    b.close()
    del b, tr, roll

    b, tr, roll = _build(**kw)                                   # fresh handles, restored
    m = roll.restore(path)
    assert m["rollout_fingerprint"]["auto_reset"] is True and m["counters"]["tick"] == half * K
    assert m["sections"]["autoreset/arena_episode"]["shape"] == [RN]
    assert m["sections"]["autoreset/dead_once"]["shape"] == [RN, ro.M]
    assert m["sections"]["rollout/auto_sums"]["shape"] == [1, ro.M + 2]
    after = _train_state(b, tr, roll)
    assert [k for k in after if after[k] != mid[k]] == []
    roll.run(half)
    got = _train_state(b, tr, roll)
    assert [k for k in got if got[k] != end[k]] == []            # names what differs; every entry is compared with ==
    b.close()
    del b, tr, roll

    b, tr, roll = _build(auto_reset=False, **kw)                 # the global clock: dead learners wait for it
    with pytest.raises(ValueError) as err:
        roll.restore(path)                                       # a checkpoint of one mode is refused by the other
    assert "rollout.auto_reset " in str(err.value)
    roll.run(2 * half)
    appended_off = int(b.replay_count()[1].sum())
    print("K = %d: appended %d with auto_reset, %d without" % (K, appended_on, appended_off))
    if K == 1:
        assert appended_on > appended_off
    b.close()
