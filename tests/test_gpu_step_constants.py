"""The lock-step (k_step, all three forms) and the rasteriser (k_raster, all five map formats) against the CPU oracle
at game constants other than the reference's own: the constant sets, rollouts, crafted boundary cases and raster scenes
of tests/step_constant_cases.py (their preconditions are checked on the CPU in tests/test_step_constant_cases.py).
Every comparison is ==.  The reference-recorded traces at changed constants (tests/golden/step_const_*.npz) are
replayed by tests/test_gpu_step.py::test_step_trace_gpu, which passes their constants into the config."""
import ctypes as C

import numpy as np
import pytest

from tests import step_constant_cases as sc

pytestmark = pytest.mark.gpu

MAP_BITS_LSB = 4     # OFX_MAP_BITS_LSB (csrc/ofx_internal.h): the format the scratch-MLP and evolution kernels read


def _nat():
    from ofighters_amd import _native as nat
    return nat


def _fields():
    nat = _nat()      # the list of test_lock_step_forms_agree_on_a_non_square_map
    return (nat.F_SHIP_X, nat.F_SHIP_Y, nat.F_SHIP_PX, nat.F_SHIP_PY, nat.F_SHIP_ALIVE, nat.F_REWARD, nat.F_SCORE,
            nat.F_OBS_REWARD, nat.F_KILLER, nat.F_HULL, nat.F_N_LASERS, nat.F_LASER_X, nat.F_LASER_Y, nat.F_LASER_DX,
            nat.F_LASER_DY, nat.F_LASER_OWNER, nat.F_LASER_DEAD, nat.F_TIME, nat.F_LAST_SCORES)


def _batch(tag, n, m, **kw):
    from ofighters_amd import ArenaBatch
    return ArenaBatch(n, m, laser_cap=64, **dict(sc.constants(tag), **kw))


def _put(b, field, arr):
    nat = _nat()
    arr = np.ascontiguousarray(arr)
    assert arr.nbytes == nat.lib().ofx_field_bytes(b.handle, field), field
    b.sync()
    nat.check(nat.lib().ofx_memcpy_h2d(nat.lib().ofx_device_ptr(b.handle, field), arr.ctypes.data_as(C.c_void_p),
                                       arr.nbytes))


def _device_states(b):
    """Per arena: the fields of sc.state() read from the device, plus obs_reward, time and the lasers' velocities."""
    nat = _nat()
    names = dict(x=nat.F_SHIP_X, y=nat.F_SHIP_Y, px=nat.F_SHIP_PX, py=nat.F_SHIP_PY, alive=nat.F_SHIP_ALIVE,
                 reward=nat.F_REWARD, score=nat.F_SCORE, killer=nat.F_KILLER, hull=nat.F_HULL,
                 last_score=nat.F_LAST_SCORES, obs_reward=nat.F_OBS_REWARD)
    ships = {k: b.get(f) for k, f in names.items()}
    nl, tm = b.get(nat.F_N_LASERS), b.get(nat.F_TIME)
    las = {k: b.get(f) for k, f in dict(lx=nat.F_LASER_X, ly=nat.F_LASER_Y, lowner=nat.F_LASER_OWNER,
                                        ldead=nat.F_LASER_DEAD, ldx=nat.F_LASER_DX, ldy=nat.F_LASER_DY).items()}
    out = []
    for g in range(b.N):
        st = {k: v[g] for k, v in ships.items()}
        n = int(nl[g])
        st.update(n_lasers=n, time=int(tm[g]), **{k: v[g, :n] for k, v in las.items()})
        out.append(st)
    return out


def _assert_state(got, want, where):
    """Every field the oracle has, with ==."""
    assert got["n_lasers"] == want["n_lasers"], where + ("n_lasers", got["n_lasers"], want["n_lasers"])
    for k in ("x", "y", "px", "py", "alive", "reward", "score", "killer", "hull", "last_score", "lx", "ly", "lowner",
              "ldead"):
        assert np.array_equal(np.asarray(got[k]).astype(np.float64), np.asarray(want[k]).astype(np.float64)), \
            where + (k, list(got[k]), list(want[k]))
    for k in ("lx", "ly"):                        # == does not tell -0.0 from 0.0
        assert np.array_equal(np.signbit(got[k]), np.signbit(want[k])), where + (k, "sign")


def _maps(b, map_type):
    """(ship maps, laser maps) of map_type as raw bytes [N][bytes of one map], freshly rasterised."""
    nat = _nat()
    b.rasterise(map_type)
    per = nat.lib().ofx_map_bytes(b.handle, map_type)
    b.sync()
    out = []
    for which in (0, 1):
        m = np.empty((b.N, per), np.uint8)
        nat.check(nat.lib().ofx_memcpy_d2h(m.ctypes.data_as(C.c_void_p),
                                           nat.lib().ofx_map_ptr(b.handle, map_type, which), m.nbytes))
        out.append(m)
    return out


def _assert_maps(b, oracles, where):
    """OFX_MAP_U8, F32, F64 and BITS against Arena.rasterise(), BITS_LSB against the same bits in little-endian order."""
    nat = _nat()
    want = [o.rasterise() for o in oracles]
    for mt, enc in ((nat.MAP_U8, lambda m: m.astype(np.uint8)), (nat.MAP_F32, lambda m: m.astype(np.float32)),
                    (nat.MAP_F64, lambda m: m.astype(np.float64)), (nat.MAP_BITS, lambda m: np.packbits(m.ravel())),
                    (MAP_BITS_LSB, sc.lsb_bits)):
        got = _maps(b, mt)
        for g in range(b.N):
            for which in (0, 1):
                w = np.ascontiguousarray(enc(want[g][which])).view(np.uint8).ravel()
                assert np.array_equal(got[which][g], w), where + (mt, g, which)


# ------------------------------------------------------------------------------------------------------- rollouts
@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_rollout_vs_oracle_and_forms_agree(tag):
    """Single calls (ofx_bot_actions + ofx_step) against the oracle after every lock-step, every field; the maps at two
    points; then ofx_rollout and ofx_step_repeat with nobody holding, as 1 + 7 + 52 lock-steps, against the single
    calls: all three instantiations of k_step at the tag's constants."""
    R = sc.ROLLOUT
    roll = sc.OracleRollout(tag)
    single, many, rep = (_batch(tag, R["N"], R["M"], arena_base=R["arena_base"]) for _ in range(3))
    for b in (single, many, rep):
        b.spawn_random(roll.seed)
    beh = list(sc.BEHAVIOURS)
    after_span = {}
    ends = set(np.cumsum(R["spans"]).tolist())
    for t in range(R["ticks"]):
        if roll.restart_due():
            roll.restart()
            single.restart_random(roll.seed)
        want_acts = roll.actions()
        single.bot_actions(beh, roll.seed, tick=t)
        acts = single.actions_host()
        single.step()
        roll.step(want_acts)
        for g in range(R["N"]):
            got = np.stack([acts[g][k] for k in ("valid", "shoot", "thrust", "px", "py")], axis=1).astype(np.int32)
            assert np.array_equal(got, want_acts[g]), (tag, t, g, "bot actions")
        for g, st in enumerate(_device_states(single)):
            _assert_state(st, sc.state(roll.oracles[g]), (tag, t, g))
            assert np.array_equal(st["obs_reward"], roll.obs_reward[g]), (tag, t, g, "obs_reward")
            assert st["time"] == roll.time, (tag, t, g, "time")
        if t + 1 in R["map_ticks"]:
            _assert_maps(single, roll.oracles, (tag, t))
        if t + 1 in ends:
            after_span[t + 1] = [single.get(f).copy() for f in _fields()]
    assert single.episode == 1 and roll.events >= sc.ROLLOUT_EVENTS[tag]
    t = 0
    for n in R["spans"]:
        for b in (many, rep):
            if t < R["restart_after"] < t + n:
                # the last span crosses the restart: run it as the lock-steps before it, the restart, and the rest
                k = R["restart_after"] - t
                (b.rollout if b is many else b.step_repeat)(beh, roll.seed, t, k)
                b.restart_random(roll.seed)
                (b.rollout if b is many else b.step_repeat)(beh, roll.seed, t + k, n - k)
            else:
                (b.rollout if b is many else b.step_repeat)(beh, roll.seed, t, n)
        t += n
        for f, want in zip(_fields(), after_span[t]):
            assert np.array_equal(many.get(f), want), (tag, t, f, "rollout")
            assert np.array_equal(rep.get(f), want), (tag, t, f, "step_repeat")
    _assert_maps(many, roll.oracles, (tag, "rollout maps"))
    for b in (single, many, rep):
        assert b.overflow_count() == 0
        b.close()


# -------------------------------------------------------------------------------------------------- crafted cases
def _plant(tag, cases):
    """One batch with one arena per case (all of M ships), planted like sc.plant() plants the oracle."""
    nat = _nat()
    N, M = len(cases), cases[0]["M"]
    b = _batch(tag, N, M)
    b.spawn(np.zeros((N, M, 2), np.int32))
    ships = np.array([c["ships"] for c in cases], np.int32)                       # [N][M][4]
    b.set_ships(x=ships[:, :, 0], y=ships[:, :, 1], px=ships[:, :, 2], py=ships[:, :, 3])
    ls = sc.TAGS[tag]["laser_speed"]
    lx, ly, ldx, ldy = (np.zeros((N, b.L)) for _ in range(4))
    lo, ld, nl = np.zeros((N, b.L), np.uint8), np.zeros((N, b.L), np.uint8), np.zeros(N, np.int32)
    for g, c in enumerate(cases):
        nl[g] = len(c["lasers"])
        for j, (x, y, dx, dy, owner, dead) in enumerate(c["lasers"]):
            lx[g, j], ly[g, j], lo[g, j], ld[g, j] = x, y, owner, dead
            ldx[g, j], ldy[g, j] = sc.device_velocity(dx, dy, ls)
    for f, a in ((nat.F_LASER_X, lx), (nat.F_LASER_Y, ly), (nat.F_LASER_DX, ldx), (nat.F_LASER_DY, ldy),
                 (nat.F_LASER_OWNER, lo), (nat.F_LASER_DEAD, ld), (nat.F_N_LASERS, nl)):
        _put(b, f, a)
    return b


@pytest.mark.parametrize("M", [2, 3])
@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_crafted_cases(tag, M):
    """All the tag's cases of M ships in one batch, two lock-steps: every field against the oracle after each, the
    hand-written expectation of each case, and all five map formats."""
    from ofighters_amd import pack_actions
    cases = [c for c in sc.crafted_cases(tag) if c["M"] == M]
    assert len(cases) >= 4
    oracles = [sc.plant(tag, c) for c in cases]
    b = _plant(tag, cases)
    for g, st in enumerate(_device_states(b)):
        _assert_state(st, sc.state(oracles[g]), (tag, cases[g]["name"], "planted"))
    _assert_maps(b, oracles, (tag, M, "planted"))
    for step in (1, 2):
        acts = np.array([c["actions"][step - 1] for c in cases], np.int32)        # [N][M][5]
        b.step(pack_actions(acts[:, :, 0], acts[:, :, 1], acts[:, :, 2], acts[:, :, 3], acts[:, :, 4]))
        for o, a in zip(oracles, acts):
            o.step(a)
        for g, st in enumerate(_device_states(b)):
            _assert_state(st, sc.state(oracles[g]), (tag, cases[g]["name"], step))
            sc.check_expectation(cases[g], step, st, vel=list(zip(st["ldx"], st["ldy"])))
        _assert_maps(b, oracles, (tag, M, step))
    assert b.overflow_count() == 0
    b.close()


@pytest.mark.parametrize("tag", sc.TAG_NAMES)
def test_raster_scene(tag):
    """Ships on every border, in every corner and past the far one, lasers centred at k + 0.5: all five formats.
    huge: discs that cover the whole map; tiny: discs of radius 1."""
    scene = sc.raster_scene(tag)
    o = sc.plant(tag, scene)
    b = _plant(tag, [scene])
    _assert_maps(b, [o], (tag, "scene"))
    sm, lm = o.rasterise()
    assert sm.any() and lm.any() and (tag != "huge" or sm.all())
    b.close()
