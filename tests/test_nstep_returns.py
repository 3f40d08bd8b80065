"""n-step returns (include/ofx.h, "n-step returns"): the CPU restatement on hand-built rows, and on the GPU the gather,
the targets and the trainer against it."""
import ctypes as C

import numpy as np
import pytest

from tests import nstep_oracle

NSTEP_SYMBOLS = ["ofx_replay_gather_nstep", "ofx_dqn_targets_nstep"]
GAMMA = 0.9


# ------------------------------------------------------------------------------------------------------ CPU
def test_nstep_symbols_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in NSTEP_SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s


def _rows(spec):
    """Hand-built memory, oldest first: spec = [(ship, tick_prev, tick_next, reward, done)]; frame slots are the ticks
    mod 7 and the heads carry the row's index, so every field tells the rows apart."""
    from ofighters_amd.engine import ArenaBatch
    rows = np.zeros(len(spec), ArenaBatch.TRANSITION_DTYPE)
    for i, (ship, tp, tn, rw, dn) in enumerate(spec):
        rows[i]["ship"], rows[i]["tick_prev"], rows[i]["tick_next"] = ship, tp, tn
        rows[i]["reward"], rows[i]["done"] = rw, dn
        rows[i]["frame_prev"], rows[i]["frame_next"] = tp % 7, tn % 7
        rows[i]["iaction"], rows[i]["px"], rows[i]["py"] = i % 2, 10 + i, 20 + i
        rows[i]["head_prev"] = np.arange(8) + 100 * i
        rows[i]["head_next"] = np.arange(8) + 100 * i + 50
    return rows


def _ret64(rewards, gamma):
    g, acc, p = float(np.float32(gamma)), 0.0, 1.0
    for r in rewards:
        acc += p * r
        p *= g
    return np.float32(acc), np.float32(p)


# ships 0 and 1 capture on every lock-step 0..6: rows alternate between them
INTERLEAVED = [(s, t, t + 1, 3 * t + s - 4, 0) for t in range(6) for s in (0, 1)]


def test_restatement_follows_the_ship_through_interleaved_rows():
    rows = _rows(INTERLEAVED)
    c = nstep_oracle.chain(rows, 1, 3, GAMMA)                  # ship 1 from lock-step 0
    assert c["idx"] == [1, 3, 5] and c["reason"] == "full" and c["L"] == 3
    assert c["ticks"] == (0, 3)
    ret, p = _ret64([rows[i]["reward"] for i in (1, 3, 5)], GAMMA)
    assert c["ret"] == ret and c["disc"] == p
    row, end = c["row"], rows[5]
    for f in ("ship", "tick_prev", "frame_prev", "iaction", "px", "py", "reward", "head_prev"):
        assert np.array_equal(row[f], rows[1][f]), f
    for f in ("tick_next", "frame_next", "done", "head_next"):
        assert np.array_equal(row[f], end[f]), f


def test_restatement_stops_at_done():
    spec = [(0, 0, 1, 1, 0), (2, 0, 1, 0, 0), (0, 1, 2, 2, 0), (2, 1, 2, 5, 0), (0, 2, 3, -7, 1), (2, 2, 3, 1, 0),
            (2, 3, 4, 1, 0)]
    rows = _rows(spec)
    c = nstep_oracle.chain(rows, 0, 8, GAMMA)
    assert c["idx"] == [0, 2, 4] and c["reason"] == "done" and c["disc"] == 0.0
    assert c["ret"] == _ret64([1, 2, -7], GAMMA)[0] and c["row"]["done"] == 1 and c["ticks"] == (0, 3)
    # done on the row itself: L = 1 whatever nstep
    c = nstep_oracle.chain(rows, 4, 5, GAMMA)
    assert c["L"] == 1 and c["reason"] == "done" and c["disc"] == 0.0 and c["ret"] == -7.0
    # done and nstep reached together: done (disc 0)
    c = nstep_oracle.chain(rows, 2, 2, GAMMA)
    assert c["idx"] == [2, 4] and c["reason"] == "done" and c["disc"] == 0.0


def test_restatement_stops_at_a_restart_and_at_the_head():
    # ship 0 plays at 0, 1, 2; the episode restarts before lock-step 3 (previous_* cleared: no row at 3); it plays on
    spec = [(0, 0, 1, 1, 0), (1, 0, 1, 0, 0), (0, 1, 2, 1, 0), (1, 1, 2, 0, 0), (0, 3, 4, 4, 0), (1, 3, 4, 0, 0),
            (0, 4, 5, 8, 0)]
    rows = _rows(spec)
    c = nstep_oracle.chain(rows, 0, 8, GAMMA)
    assert c["idx"] == [0, 2] and c["reason"] == "restart" and c["ticks"] == (0, 2)
    ret, p = _ret64([1, 1], GAMMA)
    assert c["ret"] == ret and c["disc"] == p
    c = nstep_oracle.chain(rows, 4, 8, GAMMA)                  # after the restart: up to the newest row
    assert c["idx"] == [4, 6] and c["reason"] == "head" and c["ticks"] == (3, 5)
    c = nstep_oracle.chain(rows, 5, 8, GAMMA)                  # ship 1's newest row
    assert c["idx"] == [5] and c["reason"] == "head"
    assert nstep_oracle.chain(rows, 4, 2, GAMMA)["reason"] == "full"


def test_restatement_nstep_one_is_the_one_step_row():
    rows = _rows(INTERLEAVED + [(0, 6, 7, 9, 1)])
    g32 = np.float32(GAMMA)
    for s in range(len(rows)):
        c = nstep_oracle.chain(rows, s, 1, GAMMA)
        assert c["row"].tobytes() == rows[s].tobytes() and c["L"] == 1
        assert c["ret"] == np.float32(rows[s]["reward"])
        assert c["disc"] == (np.float32(0) if rows[s]["done"] else g32)


def test_restatement_gamma_zero_and_one():
    rows = _rows(INTERLEAVED)
    c = nstep_oracle.chain(rows, 0, 4, 0.0)
    assert c["L"] == 4 and c["ret"] == rows[0]["reward"] and c["disc"] == 0.0
    c = nstep_oracle.chain(rows, 0, 4, 1.0)
    assert c["ret"] == sum(int(rows[i]["reward"]) for i in (0, 2, 4, 6)) and c["disc"] == 1.0


def test_restatement_return_is_one_rounding_of_a_float64_sum():
    # 2^24 + 1 + 1: float32 running sums stop at 2^24, the float64 sum rounded once is 2^24 + 2
    rows = _rows([(0, 0, 1, 1 << 24, 0), (0, 1, 2, 1, 0), (0, 2, 3, 1, 0)])
    c = nstep_oracle.chain(rows, 0, 3, 1.0)
    f32 = np.float32(0)
    for r in rows["reward"]:
        f32 = np.float32(f32 + np.float32(r))
    assert c["ret"] == np.float32((1 << 24) + 2) and f32 == np.float32(1 << 24)


def test_nstep_trainer_argument_checks():
    from ofighters_amd.trainer import DeviceTrainer
    w = np.zeros(4, np.float32)
    with pytest.raises(ValueError):
        DeviceTrainer(None, w, n_step=3, reference_quirks=True)
    with pytest.raises(ValueError):
        DeviceTrainer(None, w, n_step=0)


# ------------------------------------------------------------------------------------------------------ GPU
N, M, CAP, SEED = 64, 6, 50, 0x0F160051
WORDS = 400 * 400 // 32
_ROLLOUTS = {}


def _rollout(frames):
    """Random bots + device exploration (collecting phase), 3 capturing ships per arena, 150 lock-steps, episodes of
    60 lock-steps on a clock that starts 40 in (restarts at 20, 80, 140: the last one lies inside the final memory).
    Ships die, episodes restart, the rings wrap.  Kept per `frames` for the module."""
    if frames in _ROLLOUTS:
        return _ROLLOUTS[frames]
    from ofighters_amd import ArenaBatch, DeviceBuffer
    b = ArenaBatch(N, M)
    b.replay_create(CAP, frames)
    b.spawn_random(SEED)
    mask = np.zeros((N, M), np.uint8)
    mask[:, [0, 2, 5]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(150):
        if (t + 40) % 60 == 0:
            b.restart_random(SEED)
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.policy_explore(1.0, SEED, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr,
                         ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()
    # batch = capacity: the sampler draws every eligible row of every arena (in its own order)
    slot, n_s = b.replay_sample(SEED, 0, CAP)
    b.sync()
    st = dict(b=b, slot=slot, n_s=n_s, slot_h=slot.download(np.int32, (N, CAP)), n_h=n_s.download(np.int32, (N,)),
              mem=[b.replay_rows(a) for a in range(N)], frames={})
    st["entries"] = [(a, int(st["slot_h"][a, j])) for a in range(N) for j in range(st["n_h"][a])]
    _ROLLOUTS[frames] = st
    return st


@pytest.fixture(scope="module", autouse=True)
def _close_rollouts():
    yield
    for st in _ROLLOUTS.values():
        st["b"].close()
    _ROLLOUTS.clear()


def _frame(st, a, tick):
    """Packed (ship, laser) maps of a stored lock-step as uint32 [2][WORDS] (the layout the gather writes)."""
    from ofighters_amd import _native as nat
    key = (a, tick)
    if key not in st["frames"]:
        f = np.empty((2, WORDS), np.uint32)
        nat.check(nat.lib().ofx_replay_frame_host(st["b"].handle, a, tick, f[0].ctypes.data_as(C.c_void_p),
                                                   f[1].ctypes.data_as(C.c_void_p)))
        st["frames"][key] = f
    return st["frames"][key]


def _done_window(st, before):
    """A window start `before` entries ahead of the first sampled row with done != 0 (the window then holds some)."""
    k = next(k for k, (a, s) in enumerate(st["entries"]) if st["mem"][a][s]["done"])
    return max(0, k - before)


def _gather(st, first, max_rows, nstep, gamma=GAMMA, maps=True):
    from ofighters_amd import DeviceBuffer
    b = st["b"]
    rows, ret, disc = DeviceBuffer(max_rows * b.TRANSITION_DTYPE.itemsize), DeviceBuffer(4 * max_rows), DeviceBuffer(4 * max_rows)
    bp = DeviceBuffer(4 * max_rows * 2 * WORDS) if maps else None
    bn = DeviceBuffer(4 * max_rows * 2 * WORDS) if maps else None
    got = b.replay_gather_nstep_into(st["slot"], st["n_s"], CAP, first, max_rows, nstep, gamma, rows, bp, bn, ret, disc)
    out = dict(n=got, dev=(rows, bp, bn, ret, disc), rows=rows.download(b.TRANSITION_DTYPE, (got,)),
               ret=ret.download(np.float32, (got,)), disc=disc.download(np.float32, (got,)))
    if maps:
        out["bp"], out["bn"] = bp.download(np.uint32, (got, 2, WORDS)), bn.download(np.uint32, (got, 2, WORDS))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("frames", [0, 12])
def test_gather_nstep_equals_restatement(frames):
    st = _rollout(frames)
    b, entries = st["b"], st["entries"]
    total = len(entries)
    cnt, app = b.replay_count()
    assert (app > CAP).sum() > N // 2 and total > 10 * N         # the rings wrapped
    if frames:
        assert total < cnt.sum(), "the short frame ring expired no row"
    reasons = set()
    for nstep in (1, 2, 3, 8):
        # the whole sequence without the maps, and its tail with them (max_rows past the end: n_rows is clipped)
        for first, max_rows, maps in ((0, total, False), (total - 400, 1000, True)):
            g = _gather(st, first, max_rows, nstep, maps=maps)
            assert g["n"] == min(max_rows, total - first)
            for d in range(g["n"]):
                a, s = entries[first + d]
                c = nstep_oracle.chain(st["mem"][a], s, nstep, GAMMA)
                reasons.add(c["reason"])
                assert g["rows"][d].tobytes() == c["row"].tobytes(), (nstep, d, a, s, g["rows"][d], c["row"])
                assert g["ret"][d] == c["ret"] and g["disc"][d] == c["disc"], (nstep, d, g["ret"][d], c)
                if maps:
                    assert np.array_equal(g["bp"][d], _frame(st, a, c["ticks"][0])), (nstep, d)
                    assert np.array_equal(g["bn"][d], _frame(st, a, c["ticks"][1])), (nstep, d)
    assert reasons == set(nstep_oracle.REASONS), reasons
    # the walk only reads the memory
    for a in range(0, N, 7):
        assert b.replay_rows(a).tobytes() == st["mem"][a].tobytes()


def _targets(b, w_d, n, rows, bp, bn, ret=None, disc=None):
    """ofx_dqn_targets (ret None, gamma 0.9) or ofx_dqn_targets_nstep, with q_sa / p_sp: host (q_sa, p_sp, y_act, y_ptr)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    out = [DeviceBuffer(4 * n) for _ in range(4)]
    if ret is None:
        nat.check(nat.lib().ofx_dqn_targets(b.handle, w_d.ptr, n, rows.ptr, bp.ptr, bn.ptr, GAMMA, *[o.ptr for o in out]))
    else:
        nat.check(nat.lib().ofx_dqn_targets_nstep(b.handle, w_d.ptr, n, rows.ptr, bp.ptr, bn.ptr, ret.ptr, disc.ptr,
                                                   *[o.ptr for o in out]))
    b.sync()
    return [o.download(np.float32, (n,)) for o in out]


@pytest.mark.gpu
def test_nstep_one_is_the_one_step_path():
    from ofighters_amd import DeviceBuffer
    from oracle import pyoracle
    st = _rollout(0)
    b = st["b"]
    first, max_rows = _done_window(st, 96), 192
    g = _gather(st, first, max_rows, 1)
    n = g["n"]
    assert n == max_rows
    rows, bp, bn = DeviceBuffer(n * b.TRANSITION_DTYPE.itemsize), DeviceBuffer(4 * n * 2 * WORDS), DeviceBuffer(4 * n * 2 * WORDS)
    assert b.replay_gather_valid_into(st["slot"], st["n_s"], CAP, first, max_rows, rows, bp, bn) == n
    b.sync()
    assert rows.download(np.uint8, (n * b.TRANSITION_DTYPE.itemsize,)).tobytes() == g["rows"].tobytes()
    assert np.array_equal(bp.download(np.uint32, (n, 2, WORDS)), g["bp"])
    assert np.array_equal(bn.download(np.uint32, (n, 2, WORDS)), g["bn"])
    done = g["rows"]["done"] != 0
    assert 0 < done.sum() < n
    assert np.array_equal(g["ret"], g["rows"]["reward"].astype(np.float32))
    assert np.array_equal(g["disc"], np.where(done, np.float32(0), np.float32(GAMMA)))
    w, _ = pyoracle.policy_init(6, trained_like=True)
    w_d = DeviceBuffer(w.nbytes).upload(w)
    rows_n, bp_n, bn_n, ret_n, disc_n = g["dev"]
    one = _targets(b, w_d, n, rows, bp, bn)
    nst = _targets(b, w_d, n, rows_n, bp_n, bn_n, ret_n, disc_n)
    for k, name in enumerate(("q_sa", "p_sp", "y_act", "y_ptr")):
        assert one[k].tobytes() == nst[k].tobytes(), name


@pytest.mark.gpu
def test_targets_nstep_against_definition():
    from ofighters_amd import DeviceBuffer, _native as nat
    from oracle import pyoracle
    st = _rollout(0)
    b = st["b"]
    g = _gather(st, _done_window(st, 120), 160, 3)
    n = g["n"]
    g64 = float(np.float32(GAMMA))
    assert n == 160 and (g["disc"] == 0).any() and (g["disc"] == np.float32(g64 * g64 * g64)).sum() > n // 2
    w, _ = pyoracle.policy_init(7, trained_like=True)
    w_d = DeviceBuffer(w.nbytes).upload(w)
    rows_d, bp_d, bn_d, ret_d, disc_d = g["dev"]
    q_sa, p_sp, y_act, y_ptr = _targets(b, w_d, n, rows_d, bp_d, bn_d, ret_d, disc_d)
    # the forward on next_state the targets bootstrap from, called as ofx_dqn_targets_nstep calls it
    vec = DeviceBuffer(32 * n).upload(np.ascontiguousarray(g["rows"]["head_next"], np.float32))
    act, pmax = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
    nat.check(nat.lib().ofx_policy_forward_obs(b.handle, w_d.ptr, n, bn_d.ptr, vec.ptr, act.ptr, None, None, pmax.ptr,
                                                None, None))
    b.sync()
    want_act, want_ptr = nstep_oracle.targets(g["ret"], g["disc"], act.download(np.float32, (n, 2)),
                                              pmax.download(np.float32, (n,)))
    assert y_act.tobytes() == want_act.tobytes() and y_ptr.tobytes() == want_ptr.tobytes()
    # and the current values come from the composite row's state, as in ofx_dqn_targets
    q1, p1, _, _ = _targets(b, w_d, n, rows_d, bp_d, bn_d)
    assert q_sa.tobytes() == q1.tobytes() and p_sp.tobytes() == p1.tobytes()


@pytest.mark.gpu
def test_nstep_errors_leave_the_memory_alone():
    from ofighters_amd import DeviceBuffer, _native as nat
    st = _rollout(0)
    b = st["b"]
    L = nat.lib()
    cnt0, app0 = b.replay_count()
    rows, ret, disc = DeviceBuffer(64 * b.TRANSITION_DTYPE.itemsize), DeviceBuffer(256), DeviceBuffer(256)
    n = C.c_int32(-1)

    def gather(nstep, gamma, r=ret, d=disc):
        return L.ofx_replay_gather_nstep(b.handle, st["slot"].ptr, st["n_s"].ptr, CAP, 0, 64, nstep, gamma, rows.ptr, None,
                                         None, r.ptr if r else None, d.ptr if d else None, C.byref(n))
    for nstep, gamma in ((0, GAMMA), (65, GAMMA), (3, -0.1), (3, 1.5), (3, float("nan")), (3, float("inf"))):
        assert gather(nstep, gamma) == nat.OFX_ERR_INVALID, (nstep, gamma)
    assert gather(3, GAMMA, r=None) == nat.OFX_ERR_INVALID and gather(3, GAMMA, d=None) == nat.OFX_ERR_INVALID
    assert L.ofx_replay_gather_nstep(b.handle, st["slot"].ptr, st["n_s"].ptr, CAP, -1, 64, 3, GAMMA, rows.ptr, None, None,
                                     ret.ptr, disc.ptr, C.byref(n)) == nat.OFX_ERR_INVALID   # where gather_valid fails
    assert n.value == -1
    assert gather(64, 1.0) == nat.OFX_OK and gather(1, 0.0) == nat.OFX_OK and n.value == 64   # the bounds are valid
    from ofighters_amd.agents.policy_weights import synthetic
    wh = synthetic()
    w = DeviceBuffer(wh.nbytes).upload(wh)                    # full-size arguments: only ret / disc are wrong
    bits = DeviceBuffer(4 * 2 * WORDS)
    y = [DeviceBuffer(4) for _ in range(2)]
    for r, d in ((None, disc), (ret, None)):
        assert L.ofx_dqn_targets_nstep(b.handle, w.ptr, 1, rows.ptr, bits.ptr, bits.ptr, r.ptr if r else None,
                                       d.ptr if d else None, None, None, y[0].ptr, y[1].ptr) == nat.OFX_ERR_INVALID
    cnt1, app1 = b.replay_count()
    assert np.array_equal(cnt0, cnt1) and np.array_equal(app0, app1)
    for a in range(N):
        assert b.replay_rows(a).tobytes() == st["mem"][a].tobytes()


def _train(seed, n_step, prioritized=False):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    NT, MT = 32, 8
    b = ArenaBatch(NT, MT)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=8, memory_size=100, fit_batch=64,
                       seed=seed, prioritized=prioritized, n_step=n_step)
    roll = TrainingRollout(b, tr, ["random"] * MT, seed, policy_ships=(0, 1), episode_ticks=60, replay_every=5)
    roll.run(150)
    out = (tr.weights_host(), np.array(roll.losses))
    b.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("prioritized", [False, True])
def test_training_rollout_with_nstep_returns(prioritized):
    seed = 0x0F160061
    w, L = _train(seed, 3, prioritized)
    assert len(L) >= 20 and np.isfinite(L).all() and np.isfinite(w).all()
    w2, L2 = _train(seed, 3, prioritized)
    assert np.array_equal(w, w2) and np.array_equal(L, L2)
    w1, _ = _train(seed, 1, prioritized)
    assert not np.array_equal(w, w1)
