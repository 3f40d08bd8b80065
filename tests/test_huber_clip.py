"""Opt-in Huber loss and global gradient-norm clipping of the DQN fit (include/ofx.h, ofx_dqn_fit_robust): the ABI and
the trainer's argument checks on the CPU; on the GPU the entry against ofx_dqn_fit_weighted (both options off), against
a float64 torch autograd (Huber), against its own unclipped run (clip), lean against plain, and the trainer end to end."""
import ctypes as C

import numpy as np
import pytest
import torch    # before libofx.so is loaded (see tests/test_gpu_views.py): loaded between libofx.so and its first HIP call,
                # torch's own HIP runtime leaves libofx without a device when this file runs on its own

SYMBOLS = ["ofx_dqn_fit_robust"]
DELTA = 0.5


# ------------------------------------------------------------------------------------------------------ CPU
def test_robust_symbol_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    # the arguments of ofx_dqn_fit_weighted followed by huber_delta, clip_norm, grad_norm_host
    assert nat.SIGNATURES["ofx_dqn_fit_robust"][1] == \
        nat.SIGNATURES["ofx_dqn_fit_weighted"][1] + [C.c_float, C.c_float, C.c_void_p]


@pytest.mark.parametrize("name", ["huber_delta", "clip_norm"])
@pytest.mark.parametrize("value", [0, 0.0, -1.0, float("nan"), float("inf")])
def test_trainer_refuses_bad_values(name, value):
    """before it touches the batch: batch=None would fail at replay_create"""
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match=name):
        DeviceTrainer(None, np.zeros(4, np.float32), **{name: value})


@pytest.mark.parametrize("name", ["huber_delta", "clip_norm"])
def test_trainer_refuses_reference_quirks(name):
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match=name):
        DeviceTrainer(None, np.zeros(4, np.float32), reference_quirks=True, **{name: 1.0})


def test_torch_reference_huber_on_two_scalars():
    """one error in each zone, delta = 0.5: h(0.2) = 0.5 * 0.04 = 0.02 with slope 0.2; h(-2) = 0.5 * 2 - 0.125 = 0.875
    with slope -0.5"""
    from tests.fit_torch_ref import huber
    e = torch.tensor([0.2, -2.0], dtype=torch.float64, requires_grad=True)
    h = huber(e, 0.5)
    h.sum().backward()
    np.testing.assert_allclose(h.detach().numpy(), [0.02, 0.875], rtol=1e-15)
    np.testing.assert_allclose(e.grad.numpy(), [0.2, -0.5], rtol=1e-15)


# ------------------------------------------------------------------------------------------------------ GPU
def _fit_inputs(n):
    rs = np.random.RandomState(1)
    return rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)


def _row_weights(n, seed=8):
    return np.random.RandomState(seed).uniform(0.05, 1.0, n).astype(np.float32)


def _fresh(w):
    """weights, adam m, adam v, gradient"""
    from ofighters_amd import DeviceBuffer
    zeros = np.zeros_like(w)
    return [DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes).upload(zeros),
            DeviceBuffer(w.nbytes).upload(zeros)]


def _download(bufs, w):
    return [x.download(np.float32, w.shape) for x in bufs]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lean", "plain"])
def test_both_options_off_is_the_weighted_fit(form):
    from ofighters_amd import DeviceBuffer, _native as nat
    from oracle import pyoracle
    from tests.fit_cases import collect_minibatch
    b, n, rows_d, bp_d, _ = collect_minibatch(1)
    assert n == 4
    b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
    w, _ = pyoracle.policy_init(5, trained_like=True)
    y, y2 = _fit_inputs(n)
    y_d, y2_d, rw_d = (DeviceBuffer(4 * n).upload(v) for v in (y, y2, _row_weights(n)))
    res = []
    for robust in (False, True):
        bufs, td = _fresh(w), DeviceBuffer(8 * n)
        args = (bufs[0], bufs[1], bufs[2], 1, 1e-4, n, rows_d.ptr, bp_d.ptr, y_d.ptr, y2_d.ptr)
        if robust:
            l = b.dqn_fit_robust(*args, 0.0, 0.0, row_weight_ptr=rw_d.ptr, td_ptr=td.ptr, grad_buf=bufs[3])
            assert l[2] is None                             # no norm is computed: nothing but the weighted fit's launches
            l = l[:2]
        else:
            l = b.dqn_fit_weighted(*args, row_weight_ptr=rw_d.ptr, td_ptr=td.ptr, grad_buf=bufs[3])
        b.sync()
        res.append((l, _download(bufs, w) + [td.download(np.float32, (n, 2))]))
    (la, xa), (lb, xb) = res
    assert la == lb
    assert np.abs(xa[3]).max() > 0
    for k in range(5):                                      # weights, adam m, adam v, gradient, td
        assert np.array_equal(xa[k], xb[k]), k
    b.close()


_REF = {}


def _huber_case(b, n, rows_d, bp_d):
    """Targets that place the 4 rows' errors at delta * (+0.25, -0.5, +3, -2) on head 1 and a permutation of it on
    head 2 (y = o_ref - e_wanted, o_ref from the float64 graph with zero targets), random row weights, and the float64
    reference of that case.  Computed once: the collection is seeded, every caller gathers the same rows."""
    from oracle import pyoracle
    from tests.fit_torch_ref import fit_reference
    w, shapes = pyoracle.policy_init(9, trained_like=True)
    if "case" not in _REF:
        rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
        bits = bp_d.download(np.uint32, (n, 2, 5000))
        x0 = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(n, 2, 400, 400).astype(np.float64)
        fixed = (w.astype(np.float64), shapes, x0, rows["head_prev"], rows["iaction"].astype(np.int64),
                 rows["px"].astype(np.int64), rows["py"].astype(np.int64))
        rw = _row_weights(n)
        zero = np.zeros(n)
        o1, o2 = fit_reference(*fixed, zero, zero, row_w=rw, huber_delta=DELTA, backward=False)["e"].T
        want = DELTA * np.array([0.25, -0.5, 3.0, -2.0])
        y, y2 = (o1 - want).astype(np.float32), (o2 - want[[2, 0, 3, 1]]).astype(np.float32)
        ref = fit_reference(*fixed, y, y2, row_w=rw, huber_delta=DELTA)
        _REF["case"] = (y, y2, rw, (ref["l1"], ref["l2"], ref["g"], ref["e"][:, 0], ref["e"][:, 1]), rows.copy())
    y, y2, rw, ref, rows0 = _REF["case"]
    assert np.array_equal(rows_d.download(b.TRANSITION_DTYPE, (n,)), rows0)
    return w, shapes, y, y2, rw, ref


def _assert_zones(td, delta, margin):
    """the rows' errors lie in both zones on each head and none nearer than `margin` (in units of delta) to the kink"""
    r = np.abs(td.astype(np.float64)) / delta
    assert (np.abs(r - 1.0) >= margin).all(), r
    for head in (0, 1):
        assert (r[:, head] < 1).any() and (r[:, head] > 1).any(), r


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lean", "plain"])
def test_huber_fit_vs_torch_autograd(form):
    """the bounds of test_weighted_fit_vs_torch_autograd; the errors sit at |e| / delta = 0.25, 0.5, 2, 3 by
    construction, so fp32 and float64 cannot disagree on a row's zone (asserted from the returned td)"""
    from ofighters_amd import DeviceBuffer, _native as nat
    from tests.fit_cases import collect_minibatch, compare_gradients
    b, n, rows_d, bp_d, _ = collect_minibatch(1)
    assert n == 4
    b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
    w, shapes, y, y2, rw, (rl1, rl2, rg, e1, e2) = _huber_case(b, n, rows_d, bp_d)
    y_d, y2_d, rw_d = (DeviceBuffer(4 * n).upload(v) for v in (y, y2, rw))
    td_d = DeviceBuffer(8 * n)
    bufs = _fresh(w)
    l1, l2, norm = b.dqn_fit_robust(bufs[0], bufs[1], bufs[2], 1, 1e-4, n, rows_d.ptr, bp_d.ptr, y_d.ptr, y2_d.ptr,
                                    DELTA, 0.0, rw_d.ptr, td_d.ptr, bufs[3])
    b.sync()
    g = bufs[3].download(np.float32, w.shape).astype(np.float64)
    td = td_d.download(np.float32, (n, 2)).astype(np.float64)
    print("losses", l1, rl1, l2, rl2, "norm", norm, "td / delta", (td / DELTA).tolist())
    _assert_zones(td, DELTA, 0.25 - 1e-3)
    _assert_zones(np.stack([e1, e2], 1), DELTA, 0.25 - 1e-3)
    assert abs(l1 - rl1) <= 1e-4 * max(1.0, abs(rl1)) and abs(l2 - rl2) <= 1e-4 * max(1e-9, abs(rl2)) + 1e-12
    compare_gradients(shapes, rg, g)
    np.testing.assert_allclose(td[:, 0], e1, rtol=0, atol=1e-4 * max(1.0, np.abs(e1).max()))
    np.testing.assert_allclose(td[:, 1], e2, rtol=0, atol=1e-4 * max(1.0, np.abs(e2).max()))
    np.testing.assert_allclose(norm, np.sqrt((g * g).sum()), rtol=1e-6)
    b.close()


def _close(got, want, what):
    """rtol 1e-6 plus a few spacings of the fp32 value"""
    got, want = got.astype(np.float64), want.astype(np.float64)
    tol = 1e-6 * np.abs(want) + 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bad = np.abs(got - want) > tol
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


@pytest.mark.gpu
def test_gradient_norm_clip():
    """Against the entry's own unclipped run on the same 4 rows (lean form; the plain form differs only before the
    gradient).  The check goes through Adam's m and v: at step 1 from a zero state the weight update is about
    lr * sign(g), which would hide a missing scale."""
    from ofighters_amd import DeviceBuffer
    from oracle import pyoracle
    from tests.fit_cases import collect_minibatch
    b, n, rows_d, bp_d, _ = collect_minibatch(1)
    assert n == 4
    w, _ = pyoracle.policy_init(9, trained_like=True)
    y, y2 = _fit_inputs(n)
    y_d, y2_d, rw_d = (DeviceBuffer(4 * n).upload(v) for v in (y, y2, _row_weights(n)))

    def run(clip):
        bufs = _fresh(w)
        l = b.dqn_fit_robust(bufs[0], bufs[1], bufs[2], 1, 1e-4, n, rows_d.ptr, bp_d.ptr, y_d.ptr, y2_d.ptr, DELTA, clip,
                             rw_d.ptr, None, bufs[3])
        b.sync()
        return l, _download(bufs, w)

    l0, (w0, m0, v0, g0) = run(0.0)
    norm64 = float(np.sqrt((g0.astype(np.float64) ** 2).sum()))
    assert np.isfinite(norm64) and norm64 > 0
    np.testing.assert_allclose(l0[2], norm64, rtol=1e-6)
    # active: the factor from the clip_norm the entry receives (a float)
    clip = float(np.float32(0.5 * norm64))
    s = min(1.0, clip / (norm64 + 1e-6))
    assert 0.49 < s < 0.51
    l1, (w1, m1, v1, g1) = run(clip)
    print("norm64 %.9g device %.9g s %.9g" % (norm64, l1[2], s))
    assert l1[:2] == l0[:2]
    np.testing.assert_allclose(l1[2], norm64, rtol=1e-6)    # the same fp32 values summed in double: the last rounding only
    assert np.array_equal(g1, g0)                           # grad_out: the gradient before scaling
    assert np.abs(m0).max() > 0 and np.abs(v0).max() > 0
    _close(m1, s * m0.astype(np.float64), "adam_m")
    _close(v1, s * s * v0.astype(np.float64), "adam_v")
    # inactive: a factor of exactly 1
    l2, (w2, m2, v2, g2) = run(float(np.float32(2.0 * norm64)))
    assert l2 == l0
    assert np.array_equal(w2, w0) and np.array_equal(m2, m0) and np.array_equal(v2, v0) and np.array_equal(g2, g0)
    b.close()


@pytest.mark.gpu
def test_robust_lean_fit_equals_plain_fit_at_128_rows():
    """the bounds of test_lean_fit_equals_plain_fit_large_batches (its checker, reused) with huber_delta = 0.5, random
    row weights and a clip at half the gradient's norm in the textbook fit.  The checker's inputs (policy_init(5),
    RandomState(3)'s targets) are restated for one unclipped fit that gives the norm; no error of either form may lie
    within 1e-3 delta of delta, where the two forms could put a row in different zones (delta = 0.5 holds for these
    targets: the nearest error sits at 1.0026 delta in both forms, 222 of the 256 errors lie beyond delta)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    from oracle import pyoracle
    from tests.fit_cases import check_lean_equals_plain, collect_minibatch
    b, n, rows_d, bp_d, bn_d = collect_minibatch(32)
    assert n == 128
    rw = DeviceBuffer(4 * n).upload(_row_weights(n, 6))
    td_d = DeviceBuffer(8 * n)
    w, _ = pyoracle.policy_init(5, trained_like=True)
    rs = np.random.RandomState(3)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    bufs = _fresh(w)
    _, _, norm = b.dqn_fit_robust(bufs[0], bufs[1], bufs[2], 1, 1e-4, n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, DELTA, 0.0,
                                  rw.ptr, None, None)
    assert np.isfinite(norm) and norm > 0
    clip, tds, norms = 0.5 * norm, [], []

    def robust(*a, grad_buf=None):
        l1, l2, nrm = b.dqn_fit_robust(*a[:10], DELTA, clip, row_weight_ptr=rw.ptr, td_ptr=td_d.ptr,
                                       grad_buf=grad_buf if grad_buf is not None else a[10])
        b.sync()
        tds.append(td_d.download(np.float32, (n, 2)))
        norms.append(nrm)
        return l1, l2
    plain_fit = b.dqn_fit
    b.dqn_fit = robust
    try:
        check_lean_equals_plain(b, n, rows_d, bp_d, bn_d)
    finally:
        b.dqn_fit = plain_fit
    assert len(tds) == 3                                    # lean, lean again, plain
    assert np.array_equal(tds[0], tds[1]) and norms[0] == norms[1] == norm
    assert norms[0] > clip and norms[2] > clip              # the clip is active in both forms
    for td in (tds[0], tds[2]):
        r = np.abs(td.astype(np.float64)) / DELTA
        print("nearest |e| / delta to 1: %.6f; rows beyond delta: %d of %d" % (r.ravel()[np.abs(r - 1).argmin()], (r > 1).sum(), r.size))
        assert (np.abs(r - 1.0) >= 1e-3).all()
        assert (r > 1).any() and (r < 1).any()
    b.close()


# ---- end to end ------------------------------------------------------------------------------------------------------
def _train(seed, **opts):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    N, M = 64, 8
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=8, memory_size=100, fit_batch=64,
                       seed=seed, prioritized=True, per_beta_steps=40, n_step=3, **opts)
    roll = TrainingRollout(b, tr, ["idle"] * M, seed, policy_ships=(0,), episode_ticks=60, replay_every=5)
    roll.run(300)
    out = (tr.weights_host(), np.array(roll.losses), np.array(tr.grad_norms, np.float64), tr.fit_steps)
    b.close()
    return out


@pytest.mark.gpu
def test_training_rollout_with_huber_and_clip():
    """prioritized + 3-step returns + Huber(1.0); the clip sits at the median norm of the run without it, so it is
    active on about half the steps"""
    seed = 0x0F160031
    _, _, norms0, steps0 = _train(seed, huber_delta=1.0)
    assert len(norms0) == steps0 >= 50 and np.isfinite(norms0).all() and (norms0 > 0).all()
    clip = float(np.median(norms0))
    w, L, norms, steps = _train(seed, huber_delta=1.0, clip_norm=clip)
    assert len(L) >= 50 and np.isfinite(L).all()
    assert len(norms) == steps and np.isfinite(norms).all() and (norms > 0).all()
    print("clip %.4g: active on %d of %d steps" % (clip, (norms > clip).sum(), steps))
    assert (norms > clip).any() and (norms <= clip).any()
    w2, L2, norms2, _ = _train(seed, huber_delta=1.0, clip_norm=clip)
    assert np.array_equal(w, w2) and np.array_equal(L, L2) and np.array_equal(norms, norms2)
    w3, _, norms3, _ = _train(seed)
    assert len(norms3) == 0 and not np.array_equal(w, w3)


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_entry_refuses_negative_and_nan_options():
    from ofighters_amd import DeviceBuffer, _native as nat
    from oracle import pyoracle
    from tests.fit_cases import collect_minibatch
    b, n, rows_d, bp_d, _ = collect_minibatch(1)
    w, _ = pyoracle.policy_init(5, trained_like=True)
    y, y2 = _fit_inputs(n)
    y_d, y2_d = DeviceBuffer(4 * n).upload(y), DeviceBuffer(4 * n).upload(y2)
    bufs = _fresh(w)
    loss, norm = (C.c_float * 2)(), C.c_float(-1.0)
    for delta, clip in ((-0.5, 0.0), (float("nan"), 0.0), (0.0, -1.0), (0.0, float("nan")), (float("inf"), 0.0),
                        (0.0, float("inf"))):
        rc = nat.lib().ofx_dqn_fit_robust(b.handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, 1, 1e-4, n, rows_d.ptr, bp_d.ptr,
                                          y_d.ptr, y2_d.ptr, bufs[3].ptr, loss, None, None, delta, clip, C.byref(norm))
        assert rc == nat.OFX_ERR_INVALID, (delta, clip, rc)
        msg = nat.lib().ofx_last_error().decode()
        assert "ofx_dqn_fit_robust" in msg and ("huber_delta" in msg or "clip_norm" in msg), msg
    b.sync()
    got = _download(bufs, w)
    assert np.array_equal(got[0], w) and not got[1].any() and not got[2].any() and not got[3].any()
    assert norm.value == -1.0
    b.close()
