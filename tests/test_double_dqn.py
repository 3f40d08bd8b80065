"""Target network and Double DQN (include/ofx.h, "target network and Double DQN"): the CPU restatement on hand-built
arrays, and on the GPU ofx_dqn_targets_double, ofx_policy_blend_weights and the trainer's options against it."""
import ctypes as C

import numpy as np
import pytest

from tests import ddqn_oracle

DDQN_SYMBOLS = ["ofx_dqn_targets_double", "ofx_policy_blend_weights"]
GAMMA = 0.9
F = np.float32


# ------------------------------------------------------------------------------------------------------ CPU
def test_ddqn_symbols_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in DDQN_SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s


def _rows(reward, done, ship=None):
    from ofighters_amd.engine import ArenaBatch
    rows = np.zeros(len(reward), ArenaBatch.TRANSITION_DTYPE)
    rows["reward"], rows["done"] = reward, done
    rows["ship"] = 0 if ship is None else ship
    return rows


def test_restatement_selects_online_evaluates_target():
    # online prefers (1, 0, 0 by a tie, 1); the target's value there is its maximum on row 1 only
    act_online = np.array([[0.1, 0.7], [2.0, -1.0], [0.5, 0.5], [-3.0, -2.0]], F)
    act_target = np.array([[5.0, 0.25], [9.0, 1.5], [-1.0, 4.0], [7.0, -0.5]], F)
    sel = np.argmax(act_online, axis=1)                        # np.argmax: the first maximum
    assert sel.tolist() == [1, 0, 0, 1]                        # a tie selects index 0
    probe = np.array([0.5, -0.25, 2.0, 8.0], F)
    rows = _rows([3, -2, 1, 4], [0, 0, 0, 1])
    y_act, y_ptr = ddqn_oracle.targets_double(rows, GAMMA, None, None, sel, act_target, probe)
    g = F(GAMMA)
    want_act = np.array([F(3) + g * F(0.25), F(-2) + g * F(9.0), F(1) + g * F(-1.0), F(4)], F)
    want_ptr = np.array([F(3) + g * F(0.5), F(-2) + g * F(-0.25), F(1) + g * F(2.0), F(4)], F)
    assert y_act.tobytes() == want_act.tobytes() and y_ptr.tobytes() == want_ptr.tobytes()
    assert y_act[3] == 4.0 and y_ptr[3] == 4.0                 # done: the reward alone
    # never above the plain target on the target network, strictly below where the two networks disagree
    plain = rows["reward"].astype(F) + g * act_target.max(axis=1) * np.where(rows["done"] != 0, F(0), F(1))
    assert (y_act <= plain).all()
    disagree = sel != np.argmax(act_target, axis=1)
    assert disagree[:3].tolist() == [True, False, True] and (y_act[:3][disagree[:3]] < plain[:3][disagree[:3]]).all()
    # the online values themselves never enter
    other, _ = ddqn_oracle.targets_double(rows, GAMMA, None, None, sel, act_target + F(0), probe)
    assert other.tobytes() == y_act.tobytes()
    # a padding row gives zeros
    rows_p = _rows([3, -2, 1, 4], [0, 0, 0, 1], ship=[0, -1, 2, 3])
    pa, pp = ddqn_oracle.targets_double(rows_p, GAMMA, None, None, sel, act_target, probe)
    assert pa[1] == 0 and pp[1] == 0 and pa[0] == y_act[0] and pp[2] == y_ptr[2]


def test_restatement_nstep_rounds_the_product_then_the_sum():
    # disc * v = (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 rounds to 1 + 2^-11 (a tie, to even); adding ret = 2^-24 is a tie again
    # and stays there, while the fused form sees 1 + 2^-11 + 2^-23 exactly: one ulp more
    d = F(1) + F(2.0 ** -12)
    ret, disc = np.array([2.0 ** -24, 1.0], F), np.array([d, 0.0], F)
    act_target = np.array([[-5.0, d], [3.0, 4.0]], F)
    probe = np.array([d, 123.0], F)
    rows = _rows([100, 100], [0, 1])                           # reward / done / gamma are not read in this form
    y_act, y_ptr = ddqn_oracle.targets_double(rows, 0.5, ret, disc, [1, 0], act_target, probe)
    fused = F(np.float64(ret[0]) + np.float64(disc[0]) * np.float64(d))   # exact in float64, one rounding
    assert y_act[0] == F(1) + F(2.0 ** -11) and y_ptr[0] == y_act[0]
    assert fused == np.nextafter(y_act[0], F(2)) and fused != y_act[0]
    assert y_act[1] == 1.0 and y_ptr[1] == 1.0                 # disc 0 (a death inside the chain): the return alone
    with pytest.raises(ValueError):
        ddqn_oracle.targets_double(rows, 0.5, ret, None, [1, 0], act_target, probe)


def test_restatement_blend():
    src = np.array([1.0, -2.5, 3.0e-3, 7.0], F)
    dst = np.array([np.nan, np.inf, -1.0, 0.5], F)
    out = ddqn_oracle.blend(dst, src, 1.0)
    assert out.tobytes() == src.tobytes() and out is not src   # tau = 1: src exactly, even from a NaN dst
    assert ddqn_oracle.blend(dst, src, 0.0).tobytes() == dst.tobytes()
    # c * d = 0.75 (1 + 2^-23) = 0.75 + 1.5 ulp rounds to 0.75 + 2 ulp (tie, to even); tau * s = -0.5 ulp makes the sum a
    # tie again, which stays at + 2 ulp; the exact value 0.75 + 1 ulp is representable: the fused result is one ulp below
    d, s = np.array([1.0 + 2.0 ** -23], F), np.array([-(2.0 ** -23)], F)
    got = ddqn_oracle.blend(d, s, 0.25)
    exact = F(np.float64(0.75) * np.float64(d[0]) + np.float64(0.25) * np.float64(s[0]))
    assert got.dtype == F and got[0] == F(0.75) + F(2.0 ** -23)
    assert exact == np.nextafter(got[0], F(0)) and exact != got[0]
    with pytest.raises(ValueError):
        ddqn_oracle.blend(d, s, 1.5)


def test_ddqn_trainer_argument_checks():
    from ofighters_amd.trainer import DeviceTrainer
    w = np.zeros(4, np.float32)
    for kw in (dict(target_sync=3, target_tau=0.5), dict(target_sync=2.5), dict(target_sync=-1), dict(target_tau=0.0),
               dict(target_tau=1.5), dict(target_tau=-0.25), dict(target_tau=float("nan")),
               dict(target_sync=3, reference_quirks=True), dict(target_tau=0.5, reference_quirks=True),
               dict(double_dqn=True, reference_quirks=True)):
        with pytest.raises(ValueError):
            DeviceTrainer(None, w, **kw)


# ------------------------------------------------------------------------------------------------------ GPU
N, M, CAP, SEED = 64, 6, 50, 0x0F160071
WORDS = 400 * 400 // 32
_STATE = {}


def _collect(b, steps, seed, ships=(0, 2, 5), restart_phase=40):
    """Random bots + device exploration (collecting phase) on a batch whose replay memory exists: `ships` capture on
    every lock-step, episodes of 60 lock-steps on a clock that starts `restart_phase` in, so ships die and episodes
    restart inside the memory."""
    from ofighters_amd import DeviceBuffer
    n, m = b.N, b.M
    b.spawn_random(seed)
    mask = np.zeros((n, m), np.uint8)
    mask[:, list(ships)] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * n * m), DeviceBuffer(8 * n * m)
    for t in range(steps):
        if (t + restart_phase) % 60 == 0:
            b.restart_random(seed)
        b.bot_actions(["random"] * m, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr,
                         ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()


def _rollout():
    """64 arenas x 6 ships, capacity 50, 150 lock-steps; every eligible row sampled once.  Kept for the module."""
    if "st" in _STATE:
        return _STATE["st"]
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, M)
    b.replay_create(CAP, 0)
    _collect(b, 150, SEED)
    slot, n_s = b.replay_sample(SEED, 0, CAP)                  # batch = capacity: every eligible row of every arena
    b.sync()
    slot_h, n_h = slot.download(np.int32, (N, CAP)), n_s.download(np.int32, (N,))
    mem = [b.replay_rows(a) for a in range(N)]
    entries = [(a, int(slot_h[a, j])) for a in range(N) for j in range(n_h[a])]
    st = dict(b=b, slot=slot, n_s=n_s, mem=mem, entries=entries)
    _STATE["st"] = st
    return st


@pytest.fixture(scope="module", autouse=True)
def _close_rollout():
    yield
    if "st" in _STATE:
        _STATE.pop("st")["b"].close()
    _STATE.clear()


def _done_window(st, before):
    """A window start `before` entries ahead of the first sampled row with done != 0 (the window then holds some)."""
    k = next(k for k, (a, s) in enumerate(st["entries"]) if st["mem"][a][s]["done"])
    return max(0, k - before)


def _gather(st, first, n, nstep=None):
    """The window on the device: dict(rows, bp, bn[, ret, disc]) DeviceBuffers + the host rows."""
    from ofighters_amd import DeviceBuffer
    b = st["b"]
    g = dict(rows=DeviceBuffer(n * b.TRANSITION_DTYPE.itemsize), bp=DeviceBuffer(4 * n * 2 * WORDS),
             bn=DeviceBuffer(4 * n * 2 * WORDS), ret=None, disc=None)
    if nstep is None:
        got = b.replay_gather_valid_into(st["slot"], st["n_s"], CAP, first, n, g["rows"], g["bp"], g["bn"])
    else:
        g["ret"], g["disc"] = DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        got = b.replay_gather_nstep_into(st["slot"], st["n_s"], CAP, first, n, nstep, GAMMA, g["rows"], g["bp"], g["bn"],
                                         g["ret"], g["disc"])
    assert got == n
    b.sync()
    g["host"] = g["rows"].download(b.TRANSITION_DTYPE, (n,))
    return g


def _ptr(x):
    return x.ptr if x is not None else None


def _plain(b, w_d, n, g):
    """ofx_dqn_targets / ofx_dqn_targets_nstep with q_sa / p_sp: host (q_sa, p_sp, y_act, y_ptr)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    out = [DeviceBuffer(4 * n) for _ in range(4)]
    if g["ret"] is None:
        nat.check(nat.lib().ofx_dqn_targets(b.handle, w_d.ptr, n, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA,
                                             *[o.ptr for o in out]))
    else:
        nat.check(nat.lib().ofx_dqn_targets_nstep(b.handle, w_d.ptr, n, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr,
                                                   g["ret"].ptr, g["disc"].ptr, *[o.ptr for o in out]))
    b.sync()
    return [o.download(np.float32, (n,)) for o in out]


def _double(b, on_d, tg_d, n, g, current=True):
    from ofighters_amd import DeviceBuffer
    out = [DeviceBuffer(4 * n) if (current or k >= 2) else None for k in range(4)]
    b.dqn_targets_double_into(on_d.ptr, tg_d.ptr, n, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA, out[2].ptr, out[3].ptr,
                              _ptr(g["ret"]), _ptr(g["disc"]), _ptr(out[0]), _ptr(out[1]))
    b.sync()
    return [o.download(np.float32, (n,)) if o else None for o in out]


def _two_blobs():
    """Online weights, and target weights of another seed with the two units of output1 swapped (tensors 28 / 29 of
    agents/policy_weights.layout: kernel (50, 2) and bias (2,)), so that the action heads disagree."""
    from ofighters_amd.agents.policy_weights import layout
    from oracle import pyoracle
    w_on, _ = pyoracle.policy_init(6, trained_like=True)
    w_tg, _ = pyoracle.policy_init(7, trained_like=True)
    w_tg = w_tg.copy()
    off, cnt, _ = layout()
    assert cnt[28] == 100 and cnt[29] == 2
    k = w_tg[off[28]:off[28] + 100].reshape(50, 2)
    k[:] = k[:, ::-1].copy()
    w_tg[off[29]:off[29] + 2] = w_tg[off[29]:off[29] + 2][::-1].copy()
    return np.ascontiguousarray(w_on, np.float32), np.ascontiguousarray(w_tg, np.float32)


@pytest.mark.gpu
def test_same_blob_is_the_plain_path():
    from ofighters_amd import DeviceBuffer
    from oracle import pyoracle
    st = _rollout()
    b = st["b"]
    n = 192
    first = _done_window(st, 96)
    w, _ = pyoracle.policy_init(6, trained_like=True)
    w_d = DeviceBuffer(w.nbytes).upload(w)
    for nstep in (None, 3):
        g = _gather(st, first, n, nstep)
        done = g["host"]["done"] != 0
        assert 0 < done.sum() < n
        plain, dbl = _plain(b, w_d, n, g), _double(b, w_d, w_d, n, g)
        for k, name in enumerate(("q_sa", "p_sp", "y_act", "y_ptr")):
            assert np.isfinite(plain[k]).all(), name
            assert plain[k].tobytes() == dbl[k].tobytes(), (nstep, name)
        # q_sa / p_sp NULL: the same targets without the forward on `state`
        lean = _double(b, w_d, w_d, n, g, current=False)
        assert lean[2].tobytes() == dbl[2].tobytes() and lean[3].tobytes() == dbl[3].tobytes()


@pytest.mark.gpu
def test_two_blobs_against_definition():
    from ofighters_amd import DeviceBuffer, _native as nat
    st = _rollout()
    b = st["b"]
    n = 160
    g = _gather(st, _done_window(st, 120), n)
    assert 0 < (g["host"]["done"] != 0).sum() < n
    w_on, w_tg = _two_blobs()
    on_d, tg_d = DeviceBuffer(w_on.nbytes).upload(w_on), DeviceBuffer(w_tg.nbytes).upload(w_tg)
    q_sa, p_sp, y_act, y_ptr = _double(b, on_d, tg_d, n, g)
    # the definition: online on next_state for (iaction, ipointer), then the target probed at that pointer
    L = nat.lib()
    vec = DeviceBuffer(32 * n).upload(np.ascontiguousarray(g["host"]["head_next"], np.float32))
    ia, ip, act, probe = DeviceBuffer(4 * n), DeviceBuffer(8 * n), DeviceBuffer(8 * n), DeviceBuffer(4 * n)
    nat.check(L.ofx_policy_forward_obs(b.handle, on_d.ptr, n, g["bn"].ptr, vec.ptr, None, ia.ptr, ip.ptr, None, None, None))
    nat.check(L.ofx_policy_forward_obs(b.handle, tg_d.ptr, n, g["bn"].ptr, vec.ptr, act.ptr, None, None, None, ip.ptr,
                                       probe.ptr))
    b.sync()
    want_act, want_ptr = ddqn_oracle.targets_double(g["host"], GAMMA, None, None, ia.download(np.int32, (n,)),
                                                    act.download(np.float32, (n, 2)), probe.download(np.float32, (n,)))
    assert np.isfinite(want_act).all() and np.isfinite(want_ptr).all()
    assert y_act.tobytes() == want_act.tobytes() and y_ptr.tobytes() == want_ptr.tobytes()
    # neither blob alone gives these targets (a swapped or ignored blob cannot pass)
    p_on, p_tg = _plain(b, on_d, n, g), _plain(b, tg_d, n, g)
    for other in (p_on, p_tg):
        assert (y_act != other[2]).any() and (y_ptr != other[3]).any()
    # evaluating a selection never exceeds the target network's own maximum
    assert (y_act <= p_tg[2]).all() and (y_ptr <= p_tg[3]).all()
    # the current values come from the online blob
    assert q_sa.tobytes() == p_on[0].tobytes() and p_sp.tobytes() == p_on[1].tobytes()


def _forward(b, w_ptr):
    """ofx_policy_forward on the batch's current state: host (act_values, iaction, ipointer)."""
    from ofighters_amd import DeviceBuffer
    s = b.N * b.M
    act, ia, ip = DeviceBuffer(8 * s), DeviceBuffer(4 * s), DeviceBuffer(8 * s)
    b.policy_forward(w_ptr, act_ptr=act.ptr, iaction_ptr=ia.ptr, ipointer_ptr=ip.ptr)
    b.sync()
    return act.download(np.float32, (s, 2)), ia.download(np.int32, (s,)), ip.download(np.int32, (s, 2))


@pytest.mark.gpu
def test_blend_weights():
    from ofighters_amd import ArenaBatch, DeviceBuffer
    w_s, w_t = _two_blobs()
    b = ArenaBatch(8, M)
    try:
        assert b.policy_layout()[2] == w_s.size
        src, dst = DeviceBuffer(w_s.nbytes).upload(w_s), DeviceBuffer(w_t.nbytes).upload(w_t)
        want = w_t
        for _ in range(3):
            b.policy_blend_weights(dst, src, 0.25)
            want = ddqn_oracle.blend(want, w_s, 0.25)
        b.sync()
        got = dst.download(np.float32, (w_t.size,))
        assert got.tobytes() == want.tobytes()
        assert not np.array_equal(got, w_t) and not np.array_equal(got, w_s)
        assert src.download(np.float32, (w_s.size,)).tobytes() == w_s.tobytes()
        b.policy_blend_weights(dst, src, 0.0)                  # tau = 0: unchanged
        b.sync()
        assert dst.download(np.float32, (w_t.size,)).tobytes() == want.tobytes()
        nan = np.full_like(w_t, np.nan)                        # tau = 1: a copy, even over NaN
        dst.upload(nan)
        b.policy_blend_weights(dst, src, 1.0)
        b.sync()
        assert dst.download(np.float32, (w_t.size,)).tobytes() == w_s.tobytes()
        # a pinned dst is prepared again: its pinned forward is the forward of the blob it now holds
        b.spawn_random(SEED)
        dst.upload(w_t)
        b.policy_pin_weights(dst.ptr)
        before = _forward(b, dst.ptr)
        b.policy_blend_weights(dst, src, 0.25)
        pinned = _forward(b, dst.ptr)
        b.policy_pin_weights(None)
        t_h = dst.download(np.float32, (w_t.size,))
        assert t_h.tobytes() == ddqn_oracle.blend(w_t, w_s, 0.25).tobytes()
        fresh_d = DeviceBuffer(t_h.nbytes).upload(t_h)
        fresh = _forward(b, fresh_d.ptr)
        for x, y in zip(pinned, fresh):
            assert x.tobytes() == y.tobytes()
        assert before[0].tobytes() != pinned[0].tobytes()      # and the blend moved the outputs
    finally:
        b.close()


@pytest.mark.gpu
def test_ddqn_errors_modify_nothing():
    from ofighters_amd import DeviceBuffer, _native as nat
    st = _rollout()
    b = st["b"]
    L = nat.lib()
    n = 4
    g = _gather(st, 0, n, 3)
    w_on, w_tg = _two_blobs()
    on_d, tg_d = DeviceBuffer(w_on.nbytes).upload(w_on), DeviceBuffer(w_tg.nbytes).upload(w_tg)
    mark = np.full(n, -77.5, np.float32)
    out = [DeviceBuffer(4 * n).upload(mark) for _ in range(4)]

    def double(on, tg, ret, disc, outs=out):
        return L.ofx_dqn_targets_double(b.handle, _ptr(on), _ptr(tg), n, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA,
                                        _ptr(ret), _ptr(disc), *[_ptr(o) for o in outs])
    assert double(on_d, tg_d, g["ret"], None) == nat.OFX_ERR_INVALID
    assert double(on_d, tg_d, None, g["disc"]) == nat.OFX_ERR_INVALID
    assert double(None, tg_d, None, None) == nat.OFX_ERR_INVALID
    assert double(on_d, None, None, None) == nat.OFX_ERR_INVALID
    assert double(on_d, tg_d, None, None, [out[0], None, out[2], out[3]]) == nat.OFX_ERR_INVALID   # q_sa without p_sp
    assert double(on_d, tg_d, None, None, [None, None, None, out[3]]) == nat.OFX_ERR_INVALID

    def blend(dst, src, tau):
        return L.ofx_policy_blend_weights(b.handle, _ptr(dst), _ptr(src), tau)
    for tau in (-0.1, 1.5, float("nan"), float("inf"), -float("inf")):
        assert blend(tg_d, on_d, tau) == nat.OFX_ERR_INVALID, tau
    assert blend(tg_d, tg_d, 0.5) == nat.OFX_ERR_INVALID
    assert blend(None, on_d, 0.5) == nat.OFX_ERR_INVALID and blend(tg_d, None, 0.5) == nat.OFX_ERR_INVALID
    assert L.ofx_policy_blend_weights(None, tg_d.ptr, on_d.ptr, 0.5) == nat.OFX_ERR_INVALID
    b.sync()
    for o in out:
        assert o.download(np.float32, (n,)).tobytes() == mark.tobytes()
    assert on_d.download(np.float32, (w_on.size,)).tobytes() == w_on.tobytes()
    assert tg_d.download(np.float32, (w_tg.size,)).tobytes() == w_tg.tobytes()
    # and the valid calls next to them pass
    assert double(on_d, tg_d, g["ret"], g["disc"]) == nat.OFX_OK and double(on_d, tg_d, None, None) == nat.OFX_OK
    assert blend(tg_d, on_d, 0.0) == nat.OFX_OK and blend(tg_d, on_d, 1.0) == nat.OFX_OK
    b.sync()


NT, MT, CAPT = 32, 6, 50


def _trainer(seed, **kw):
    """A 32-arena batch with a filled replay memory and a DeviceTrainer on it (fit_batch 32)."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(NT, MT)
    w0 = synthetic(7)
    tr = DeviceTrainer(b, w0, learning_rate=1e-3, batch_size=8, memory_size=CAPT, fit_batch=32, seed=seed, **kw)
    _collect(b, 40, seed, ships=(0, 3), restart_phase=30)
    return b, tr, w0


@pytest.mark.gpu
def test_trainer_target_sync_schedule():
    b, tr, w0 = _trainer(0x0F160072, target_sync=3)
    try:
        assert tr.target_host().tobytes() == w0.tobytes()
        snaps, targets = [w0], [w0]
        for _ in range(7):
            loss = tr.replay()
            assert loss is not None and np.isfinite(loss).all()
            snaps.append(tr.weights_host())
            targets.append(tr.target_host())
        for r in range(1, 8):
            assert not np.array_equal(snaps[r], snaps[r - 1]), r            # the fit moved the online weights
            want = snaps[(r // 3) * 3]                                      # initial, after replay 3, after replay 6
            assert targets[r].tobytes() == want.tobytes(), r
    finally:
        b.close()
    b, tr, w0 = _trainer(0x0F160072, target_tau=0.25)
    try:
        prev = w0
        for r in range(1, 5):
            assert tr.replay() is not None
            want = ddqn_oracle.blend(prev, tr.weights_host(), 0.25)
            prev = tr.target_host()
            assert prev.tobytes() == want.tobytes(), r
        assert not np.array_equal(prev, w0)
    finally:
        b.close()
    b, tr, w0 = _trainer(0x0F160072)
    try:
        assert tr.target_host() is None and tr.target is None
    finally:
        b.close()


@pytest.mark.gpu
def test_trainer_targets_come_from_the_target_blob():
    seed = 0x0F160073
    losses = []
    for kw in (dict(), dict(double_dqn=True, target_sync=10 ** 9)):
        b, tr, w0 = _trainer(seed, **kw)
        try:
            losses.append([tr.replay() for _ in range(4)])
            if kw:
                assert tr.target_host().tobytes() == w0.tobytes()          # the target never moved
        finally:
            b.close()
    plain, frozen = losses
    assert np.isfinite(np.array(plain)).all() and np.isfinite(np.array(frozen)).all()
    # target == online at the first replay: the same targets, and fits are reproducible to the bit
    assert np.array(plain[0], np.float32).tobytes() == np.array(frozen[0], np.float32).tobytes()
    for r in range(1, 4):
        assert plain[r][0] != frozen[r][0] and plain[r][1] != frozen[r][1], r
    b, tr, _ = _trainer(seed, double_dqn=True, target_sync=2, prioritized=True, n_step=3)
    try:
        out = [tr.replay() for _ in range(4)]
        assert all(o is not None for o in out) and np.isfinite(np.array(out)).all()
        assert tr.target_host().tobytes() == tr.weights_host().tobytes()   # synced after fit steps 2 and 4
    finally:
        b.close()
