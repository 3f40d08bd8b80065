"""The exploration ladder and the evaluation arenas on the device: ofx_policy_explore / ofx_policy_act under a ladder against
tests/ladder_oracle.py, the grouped episode scores against numpy, sharding, and a TrainingRollout with both options -
what it captures, what it logs, and its checkpoint."""
import ctypes as C

import numpy as np
import pytest

from tests import ladder_oracle as lo

pytestmark = pytest.mark.gpu

W = H = 400
INF = float("inf")


def _base(N, M, seed):
    """Arbitrary greedy results to explore over: no forward is needed to test the draw."""
    rs = np.random.RandomState(seed)
    ia = rs.randint(0, 2, (N, M)).astype(np.int32)
    ip = np.stack([rs.randint(0, W, (N, M)), rs.randint(0, H, (N, M))], -1).astype(np.int32)
    return ia, ip


class _Explorer:
    """policy_explore over uploaded base results on one handle: numpy in, numpy out."""

    def __init__(self, b, seed=5):
        from ofighters_amd import DeviceBuffer
        self.b, S = b, b.N * b.M
        self.ia, self.ip = _base(b.N, b.M, seed)
        self.dia, self.dip, self.dmask = DeviceBuffer(4 * S), DeviceBuffer(8 * S), DeviceBuffer(S)

    def __call__(self, eps, tick, collecting=False, mask=None, rng_seed=lo.SEED):
        b = self.b
        b.sync()
        self.dia.upload(self.ia), self.dip.upload(self.ip)
        if mask is not None:
            self.dmask.upload(np.ascontiguousarray(mask, np.uint8))
        b.policy_explore(eps, rng_seed, tick=tick, collecting=collecting, ship_mask_ptr=self.dmask.ptr if mask is not None else None,
                         iaction_ptr=self.dia.ptr, ipointer_ptr=self.dip.ptr)
        b.sync()
        return self.dia.download(np.int32, (b.N, b.M)), self.dip.download(np.int32, (b.N, b.M, 2))


def _same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# --------------------------------------------------------------------------------- 1. explore against the oracle
def test_explore_under_a_ladder_equals_the_oracle():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    from oracle import pyoracle
    N, M, L = lo.N, lo.M, lo.N - lo.EVAL
    ex = lo.ladder()
    zero = ex.copy()
    zero[5] = 0.0                                                   # exponent 0: pow(0, 0) = 1, the arena always explores
    assert lo.flip_distance(lo.EPSILONS, ex) >= 1e-4 and lo.flip_distance((0.0, 1.0), zero) == 1.0   # no ship left out
    b = ArenaBatch(N, M, arena_base=lo.ARENA_BASE)
    b.spawn_random(lo.SEED)
    run = _Explorer(b)
    some = ((np.arange(N)[:, None] + np.arange(M)[None, :]) % 3 != 0).astype(np.uint8)   # clears ships of every arena
    assert (some == 0).any(axis=1).all() and (some == 1).any(axis=1).all()
    b.policy_epsilon_ladder(ex)
    assert b.policy_epsilon_ladder_host().tobytes() == ex.tobytes()
    seen = []
    for eps, tick, collecting, mask, expo in ((0.4, 7, False, None, ex), (0.9, 8, False, None, ex), (1.0, 9, False, None, ex),
                                              (0.0, 10, False, None, zero), (0.4, 11, True, None, ex),
                                              (0.9, 12, False, some, ex)):
        if expo is not ex:
            b.policy_epsilon_ladder(expo)
        hit, play = lo.explore(pyoracle, M, eps, expo, lo.SEED, lo.ARENA_BASE, tick, collecting)
        got = run(eps, tick, collecting, mask)
        assert _same(got, lo.expected(run.ia, run.ip, hit, play, mask)), (eps, tick, collecting)
        assert not hit[L:].any()                                    # the greedy arenas, the collecting phase included
        if eps == 1.0 or collecting:
            assert hit[:L].all()
        if eps == 0.0:
            assert hit[5].all() and hit.sum() == M
        if mask is not None:
            assert (hit & (mask == 0)).any() and np.array_equal(got[0][mask == 0], run.ia[mask == 0])
        if expo is not ex:
            b.policy_epsilon_ladder(ex)
        seen.append(int(hit.sum()))
    assert 0 < seen[0] < seen[1] < seen[2] == L * M, seen
    # without the ladder again: the scalar rule, the same draws
    b.policy_epsilon_ladder(None)
    with pytest.raises(OfxError) as err:
        b.policy_epsilon_ladder_host()
    assert err.value.code == nat.OFX_ERR_STATE
    for eps, tick in ((0.4, 13), (0.9, 14)):
        hit, play = lo.scalar(pyoracle, N, M, eps, lo.SEED, lo.ARENA_BASE, tick)
        assert hit[L:].any() and _same(run(eps, tick), lo.expected(run.ia, run.ip, hit, play))
    b.close()


# ------------------------------------------------------------------------------ 2. an all-ones ladder is no ladder
def test_all_ones_ladder_equals_no_ladder():
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(lo.N, lo.M, arena_base=lo.ARENA_BASE)
    b.spawn_random(lo.SEED)
    run = _Explorer(b)
    cases = [(0.4, 7, False), (0.9, 8, False), (1.0, 9, False), (0.0, 10, False), (0.4, 11, True)]
    plain = [run(*c) for c in cases]
    b.policy_epsilon_ladder(np.ones(lo.N))
    ones = [run(*c) for c in cases]
    for c, p, o in zip(cases, plain, ones):
        assert p[0].tobytes() == o[0].tobytes() and p[1].tobytes() == o[1].tobytes(), c
    assert not _same(plain[0], plain[1]) and not _same(plain[0], (run.ia, run.ip))     # the cases do explore
    b.close()


# ------------------------------------------------------------------- 3. act == forward + explore, under a ladder
def test_act_under_a_ladder_equals_forward_plus_explore():
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.exploration import apex_exponents
    from oracle import pyoracle
    N, M, SEED, EPS = 6, 5, 0x0F160041, 0.9
    S = N * M
    ex = apex_exponents(N, 7.0, 0, N, eval_arenas=2)                # 1, 3.33, 5.67, 8, then two greedy arenas
    assert lo.flip_distance((EPS,), ex) >= 1e-4
    a, b = ArenaBatch(N, M), ArenaBatch(N, M)
    w = synthetic(7)
    dw = DeviceBuffer(w.nbytes).upload(w)
    for e in (a, b):
        e.spawn_random(SEED)
        e.policy_epsilon_ladder(ex)
    vals = [DeviceBuffer(4 * S) for _ in range(4)]
    act_d, ia_d, ip_d = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S)
    explored = greedy = 0
    for tick, collecting in ((0, 0), (1, 0), (2, 1)):
        for e in (a, b):
            e.bot_actions(["random"] * M, SEED, tick=tick)
        a.policy_act(dw.ptr, EPS, SEED, tick=tick, collecting=collecting, q_sa_ptr=vals[0].ptr, p_sp_ptr=vals[1].ptr,
                     v_act_ptr=vals[2].ptr, v_ptr_ptr=vals[3].ptr)
        a.policy_actions()
        b.policy_forward(dw.ptr)
        b.policy_explore(EPS, SEED, tick=tick, collecting=collecting)
        b.policy_actions()
        got, want = a.actions_host(), b.actions_host()
        assert got.tobytes() == want.tobytes()                      # (iaction, ipointer), bit for bit
        b.policy_forward(dw.ptr, None, act_d.ptr, ia_d.ptr, ip_d.ptr)
        b.sync(), a.sync()
        act = act_d.download(np.float32, (N, M, 2))
        q_sa, p_sp, v_act, v_ptr = (v.download(np.float32, (N, M)) for v in vals)
        hit, play = lo.explore(pyoracle, M, EPS, ex, SEED, 0, tick, collecting)
        ia = want["thrust"].astype(np.int64)
        assert np.array_equal(want["shoot"], 1 - ia)
        assert np.array_equal(q_sa, np.take_along_axis(act, ia[..., None], -1)[..., 0])
        assert np.array_equal(v_act, act.max(-1))
        assert np.array_equal(p_sp[~hit], v_ptr[~hit]) and not hit[4:].any() and np.array_equal(p_sp[4:], v_ptr[4:])
        assert np.array_equal(ia[hit], play[hit][:, 0]) and np.array_equal(want["px"][hit], play[hit][:, 1])
        assert np.array_equal(want["py"][hit], play[hit][:, 2])
        assert np.array_equal(ia[~hit], ia_d.download(np.int32, (N, M))[~hit])
        if collecting:
            assert hit[:4].all()
        explored += int(hit.sum())
        greedy += int((~hit[:4]).sum())
        a.step(), b.step()
    assert explored >= 4 * M + 4 and greedy >= 4, (explored, greedy)
    a.close(), b.close()


# ------------------------------------------------------------------------------------------------ 4. error codes
def test_error_codes_leave_the_ladder_unchanged():
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    N, M = 5, 3
    L = nat.lib()
    b = ArenaBatch(N, M)
    b.spawn_random(1)
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)
    out = np.zeros(N, np.float64)
    assert L.ofx_policy_epsilon_ladder_host(b.handle, ptr(out)) == nat.OFX_ERR_STATE          # before the first set
    good = np.array([1.0, 0.0, 2.5, INF, 8.0])
    assert L.ofx_policy_epsilon_ladder(b.handle, ptr(good)) == nat.OFX_OK
    for bad in (np.array([1.0, 2.0, np.nan, 1.0, 1.0]), np.array([1.0, 2.0, 3.0, 4.0, -1e-9]), np.array([-INF, 1, 1, 1, 1.0])):
        assert L.ofx_policy_epsilon_ladder(b.handle, ptr(bad)) == nat.OFX_ERR_INVALID
        assert L.ofx_last_error().startswith(b"ofx_policy_epsilon_ladder")
        assert b.policy_epsilon_ladder_host().tobytes() == good.tobytes()
    assert L.ofx_policy_epsilon_ladder(None, ptr(good)) == nat.OFX_ERR_INVALID
    assert L.ofx_policy_epsilon_ladder_host(None, ptr(out)) == nat.OFX_ERR_INVALID
    assert L.ofx_policy_epsilon_ladder_host(b.handle, None) == nat.OFX_ERR_INVALID
    assert b.policy_epsilon_ladder_host().tobytes() == good.tobytes()
    with pytest.raises(ValueError):
        b.policy_epsilon_ladder(np.ones(N + 1))
    # a ladder does not relax the checks of epsilon
    for call in (lambda: b.policy_explore(1.5, 1, tick=0), lambda: b.policy_explore(-0.1, 1, tick=0)):
        with pytest.raises(nat.OfxError) as err:
            call()
        assert err.value.code == nat.OFX_ERR_INVALID
    # the grouped scores
    grp, sums = DeviceBuffer(4 * N).upload(np.zeros(N, np.int32)), DeviceBuffer(8 * N * (M + 1))
    for args in ((None, grp.ptr, 1, sums.ptr), (b.handle, None, 1, sums.ptr), (b.handle, grp.ptr, 1, None),
                 (b.handle, grp.ptr, 0, sums.ptr), (b.handle, grp.ptr, -3, sums.ptr), (b.handle, grp.ptr, N + 1, sums.ptr)):
        assert L.ofx_episode_scores_grouped(*args) == nat.OFX_ERR_INVALID, args
        assert L.ofx_last_error().startswith(b"ofx_episode_scores_grouped")
    assert L.ofx_episode_scores_grouped(b.handle, grp.ptr, N, sums.ptr) == nat.OFX_OK
    b.sync()
    got = sums.download(np.int64, (N, M + 1))
    assert got[0].tolist() == [0] * M + [N] and not got[1:].any()                             # nothing banked yet
    b.close()


# --------------------------------------------------------------------------------------------- 5. grouped scores
def _episode(b, seed, ticks, first_arena=0):
    """One short episode of turrets packed into a 60 x 60 box - so close that their shots find an enemy on the
    trajectory, which is what scores - and the restart that banks the scores.  The box is keyed by the global arena."""
    rs = np.random.RandomState(seed)
    xy = rs.randint(170, 231, (first_arena + b.N, b.M, 2))[first_arena:].astype(np.int32)
    b.set_ships(x=xy[..., 0], y=xy[..., 1])
    for t in range(ticks):
        b.bot_actions(["turret"] * b.M, seed, tick=t)
        b.step()
    b.restart_random(seed)


def _grouped_numpy(last, group, G):
    out = np.zeros((G, last.shape[1] + 1), np.int64)
    for a, g in enumerate(group):
        if 0 <= g < G:
            out[g, :-1] += last[a]
            out[g, -1] += 1
    return out


@pytest.mark.parametrize("N,M,ticks", [(12, 3, 30), (300, 2, 30)])       # one pass of the block / arenas beyond its 256 threads
def test_grouped_scores_equal_numpy(N, M, ticks):
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.exploration import score_groups
    b = ArenaBatch(N, M)
    b.spawn_random(21)
    _episode(b, 21, ticks)
    last = b.get(nat.F_LAST_SCORES).astype(np.int64)
    assert len(set(last.sum(1).tolist())) > 1, "the episode banked nothing to tell arenas apart"
    full = score_groups(N, 0, N, 3, 0)
    buf = DeviceBuffer(4 * N)
    total = b.episode_scores()
    got = b.episode_scores_grouped(buf.upload(full), 3)
    assert got.dtype == np.int64 and np.array_equal(got, _grouped_numpy(last, full, 3))
    assert np.array_equal(got.sum(0), total) and got[:, -1].sum() == N
    holes = full.copy()
    holes[7] = -1
    b.sync()
    got = b.episode_scores_grouped(buf.upload(holes), 3)
    assert np.array_equal(got, _grouped_numpy(last, holes, 3)) and got[:, -1].sum() == N - 1
    holes[0], holes[N - 1], holes[3] = 3, -7, 2**31 - 1             # outside [-1, n_groups): ignored like -1
    b.sync()
    got = b.episode_scores_grouped(buf.upload(holes), 3)
    assert np.array_equal(got, _grouped_numpy(last, holes, 3)) and got[:, -1].sum() == N - 4
    b.sync()
    got = b.episode_scores_grouped(buf.upload(np.arange(N, dtype=np.int32)), N)        # a group per arena
    assert np.array_equal(got[:, :-1], last) and (got[:, -1] == 1).all()
    # crafted scores: negative ones, and sums that leave int32
    rs = np.random.RandomState(N)
    made = rs.randint(-2**31, 2**31, (N, M), dtype=np.int64).astype(np.int32)
    made[:, 0] = 2**31 - 1 - np.arange(N)
    nat.check(nat.lib().ofx_memcpy_h2d(b.device_ptr(nat.F_LAST_SCORES), made.ctypes.data_as(C.c_void_p), made.nbytes))
    got = b.episode_scores_grouped(buf.upload(holes), 3)
    want = _grouped_numpy(made.astype(np.int64), holes, 3)
    assert np.array_equal(got, want) and want[:, 0].max() > 2**32
    b.close()


# --------------------------------------------------------------------------------------------------- 6. sharding
def test_two_shards_equal_one_batch():
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.exploration import apex_exponents, score_groups
    M, TOTAL, EVAL, SEED, G = 4, 8, 2, 31, 3
    ia, ip = _base(TOTAL, M, 9)
    out = {}
    for name, base, n in (("whole", 0, 8), ("low", 0, 4), ("high", 4, 4)):
        b = ArenaBatch(n, M, arena_base=base)
        b.spawn_random(SEED)
        b.policy_epsilon_ladder(apex_exponents(TOTAL, 7.0, base, n, EVAL))
        run = _Explorer(b)
        run.ia, run.ip = ia[base:base + n], ip[base:base + n]
        acts = [run(eps, tick, rng_seed=SEED) for eps, tick in ((0.9, 3), (0.6, 4))]
        _episode(b, SEED, 30, first_arena=base)
        grp = DeviceBuffer(4 * n).upload(score_groups(TOTAL, base, n, 2, EVAL))
        out[name] = (acts, b.episode_scores_grouped(grp, G), b.episode_scores())
        b.close()
    for k in range(2):
        for j in range(2):
            assert np.array_equal(np.concatenate([out["low"][0][k][j], out["high"][0][k][j]]), out["whole"][0][k][j])
    assert not np.array_equal(out["whole"][0][0][0], ia)                                # something explored
    assert np.array_equal(out["low"][1] + out["high"][1], out["whole"][1])
    assert out["whole"][1][:, -1].tolist() == [3, 3, 2] and out["high"][1][:, -1].tolist() == [0, 2, 2]
    assert np.array_equal(out["whole"][1].sum(0), out["whole"][2]) and out["whole"][1][:, :-1].any()


# ------------------------------------------------------------------------------------------ 7. / 8. the rollout
N7, M7, SEED7, TICKS7, STEPS7 = 8, 3, 0x0F160043, 12, 25


def _build(actor=False, **roll_kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N7, M7)
    eps = Epsilon_decay()
    eps.set(0.6)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=8,
                       prioritized=actor, actor_priorities=actor)
    roll = TrainingRollout(b, tr, ["random"] * M7, SEED7, policy_ships=(0, 1), episode_ticks=TICKS7, collecting_steps=3,
                           replay_every=3, **roll_kw)
    return b, tr, roll


def _memory(b, ticks):
    from ofighters_amd import OfxError
    cnt, app = b.replay_count()
    frames = []
    for a in range(b.N):
        held = {}
        for t in range(ticks):
            try:
                s, l = b.replay_frame(a, t)
                held[t] = (np.packbits(s).tobytes(), np.packbits(l).tobytes())
            except OfxError:
                pass
        frames.append(held)
    return cnt.tobytes(), app.tobytes(), [b.replay_rows(a).tobytes() for a in range(b.N)], frames


def _state(b, tr, roll):
    b.sync()
    return dict(weights=tr.weights_host().tobytes(), memory=_memory(b, roll.capture_tick), fit_steps=tr.fit_steps,
                rung_log=[g.tolist() for g in roll.rung_log], score_log=[s.tolist() for s in roll.score_log],
                losses=list(roll.losses), state=[b.get(f).tobytes() for f in range(19)], epsilon=tr.epsilon.get())


LADDER = dict(epsilon_ladder=7.0, eval_arenas=2)
_RUNS = {}


def _run(key, actor=False, **roll_kw):
    """A run of STEPS7 lock-steps, once per configuration."""
    if key not in _RUNS:
        b, tr, roll = _build(actor, **roll_kw)
        roll.run(STEPS7)
        b.sync()
        cnt, _ = b.replay_count()
        _RUNS[key] = dict(_state(b, tr, roll), count=cnt.copy(), loss=tr.replay(), eval_scores=list(roll.eval_scores),
                          expo=b.policy_epsilon_ladder_host() if roll.ladder_on else None, n_groups=getattr(roll, "n_groups", 0))
        b.close()
    return _RUNS[key]


@pytest.mark.parametrize("actor", [False, True])
def test_rollout_with_a_ladder_and_evaluation_arenas(actor):
    from ofighters_amd.exploration import apex_exponents
    r = _run(("ladder", actor), actor, **LADDER)
    assert r["expo"].tobytes() == apex_exponents(N7, 7.0, 0, N7, 2).tobytes()
    assert (r["count"][N7 - 2:] == 0).all() and (r["count"][:N7 - 2] > 0).all(), r["count"]
    assert r["loss"] is not None and len(r["loss"]) == 2 and np.isfinite(r["loss"]).all()
    assert r["fit_steps"] >= 3 and len(r["losses"]) >= 3
    assert len(r["rung_log"]) == 2 == len(r["score_log"]) and r["n_groups"] == 7          # 6 bands of one arena, the eval group
    for g, s in zip(r["rung_log"], r["score_log"]):
        g = np.array(g)
        assert g.shape == (7, M7 + 1) and np.array_equal(g.sum(0), s) and g[:, -1].tolist() == [1] * 6 + [2]
    assert len(r["eval_scores"]) == 2
    assert r["eval_scores"] == [(g[-1][0] + g[-1][1]) / 4.0 for g in r["rung_log"]]


def test_rollout_with_an_all_ones_ladder_equals_the_default():
    off, ones = _run("off"), _run("ones", epsilon_ladder=0.0, eval_arenas=0)
    assert ones["expo"].tolist() == [1.0] * N7 and off["expo"] is None
    for k in ("weights", "memory", "fit_steps", "score_log", "losses", "state", "epsilon"):
        assert ones[k] == off[k], k
    assert off["rung_log"] == [] and len(ones["rung_log"]) == 2 and (off["count"] > 0).all()
    assert all(np.array_equal(np.array(g).sum(0), s) for g, s in zip(ones["rung_log"], ones["score_log"]))
    assert off["weights"] != _run(("ladder", False), False, **LADDER)["weights"]        # the options do change a run


def test_checkpoint_resume_under_the_options_is_bit_identical(tmp_path):
    ref = _run(("ladder", False), False, **LADDER)
    b, tr, roll = _build(**LADDER)
    roll.run(14)                                                    # past the first episode end, mid-episode
    assert tr.fit_steps >= 2 and len(roll.rung_log) == 1
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    b.close()
    del b, tr, roll
    b, tr, roll = _build(**LADDER)
    man = roll.restore(path)
    assert man["sections"]["rollout/rung_log"]["shape"] == [1, 7, M7 + 1]
    assert man["rollout_fingerprint"]["epsilon_ladder"] == 7.0 and man["rollout_fingerprint"]["eval_arenas"] == 2
    roll.run(STEPS7 - 14)
    end = _state(b, tr, roll)
    assert [k for k in end if end[k] != ref[k]] == []
    b.close()
    b, tr, roll = _build()                                          # a run without the options refuses it
    with pytest.raises(ValueError, match="rollout.eval_arenas"):
        roll.restore(path)
    b.close()
