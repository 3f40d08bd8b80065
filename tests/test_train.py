"""ofx_dqn_fit (one model.fit step of Trainer.replay) against torch autograd: the same graph in
training mode (BatchNorm on batch statistics), the same loss (mse on both heads with one non-zero error per head and
sample), float64 on the CPU as the checker.  Keras itself is absent from the image: parity with it is UNPINNED, the
conventions are those declared in ofighters_amd/csrc/ofx_train.hip."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.fit_cases import batch_statistics_f64, check_lean_equals_plain, collect_minibatch, compare_gradients, fit_once
from tests.fit_torch_ref import fit_reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", ["lean", "plain"])
@pytest.mark.parametrize("legacy", [False, True])
def test_dqn_fit_vs_torch_autograd(legacy, form):
    """legacy: OFX_OPT_BILINEAR_LEGACY - the fit's up-sampling (forward and backward) follows the same switch.
    form: the lean fit (default: only z of every convolution kept, the rest recomputed in fused tiles, ofx_fit.hip) and the
    plain layer-by-layer form (OFX_OPT_FIT_PLAIN) are both checked against the float64 graph."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    N, M, seed, batch, lr = 2, 4, 0x0F160001, 2, 1e-4
    b = ArenaBatch(N, M)
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
    b.replay_create(16, 0)
    b.spawn_random(seed)
    w, shapes = pyoracle.policy_init(9, trained_like=True)
    mask = np.zeros((N, M), np.uint8)
    mask[:, [0, 2]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(12):
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    slot, _ = b.replay_sample(3, 0, batch)
    rows_d, bp_d, bn_d = b.replay_gather_device(slot, batch)
    b.sync()                                                # the gather runs on the handle's stream; raw copies do not wait for it
    n = N * batch
    rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
    assert (rows["ship"] >= 0).all()
    rs = np.random.RandomState(1)
    y_act, y_ptr = rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)
    b.sync()
    ya_d, yp_d = DeviceBuffer(4 * n).upload(y_act), DeviceBuffer(4 * n).upload(y_ptr)
    w_d = DeviceBuffer(w.nbytes).upload(w)
    zeros = np.zeros_like(w)
    m_d, v_d, g_d = DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes)
    l1, l2 = b.dqn_fit(w_d, m_d, v_d, 1, lr, n, rows_d.ptr, bp_d.ptr, ya_d.ptr, yp_d.ptr, g_d)
    g = g_d.download(np.float32, w.shape).astype(np.float64)
    w_new = w_d.download(np.float32, w.shape)

    bits = bp_d.download(np.uint32, (n, 2, 5000))
    x0 = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(n, 2, 400, 400).astype(np.float64)
    ref = fit_reference(w.astype(np.float64), shapes, x0, rows["head_prev"], rows["iaction"].astype(np.int64),
                        rows["px"].astype(np.int64), rows["py"].astype(np.int64), y_act, y_ptr, legacy=legacy)
    rl1, rl2, rg, stats = ref["l1"], ref["l2"], ref["g"], ref["stats"]
    assert abs(l1 - rl1) <= 1e-4 * max(1.0, abs(rl1)) and abs(l2 - rl2) <= 1e-4 * max(1e-9, abs(rl2)) + 1e-12
    compare_gradients(shapes, rg, g)
    # Adam step 1 from the device's own gradient, and the moving statistics
    lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
    for name, (o, shp) in shapes.items():
        c = int(np.prod(shp))
        layer, kind = name.split(".")
        if kind in ("mean", "var"):
            bm, bv = stats[layer]
            want = 0.99 * w[o:o + c] + 0.01 * (bm if kind == "mean" else bv)
            np.testing.assert_allclose(w_new[o:o + c], want, rtol=1e-4, atol=1e-6)
        else:
            gi = g[o:o + c]
            want = w[o:o + c] - lr_t * (0.1 * gi) / (np.sqrt(0.001 * gi * gi) + 1e-7)
            np.testing.assert_allclose(w_new[o:o + c], want, rtol=0, atol=2e-7 + 1e-6 * np.abs(w[o:o + c]).max())
    b.close()


@pytest.mark.parametrize("form", ["lean", "plain"])
def test_dqn_fit_reference_quirks(form):
    """ofx_dqn_fit_reference = Trainer.replay as written (qlearnIA_V2.py:251-285): targets are float64 predictions of
    `state` (tests/policy_ref64.py) with target[iaction] and ptr_target[x][y] (row x, column y - the quirk) replaced by
    reward + gamma * max(prediction(next_state)) * (not done); the fit runs in training mode on NEXT_state's maps and
    head; dense mse on both outputs.  Checked against torch autograd in float64, like the textbook step above."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from tests import policy_ref64 as R
    N, M, seed, batch, lr, gamma = 2, 4, 0x0F160001, 2, 1e-4, 0.9
    b = ArenaBatch(N, M)
    b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
    b.replay_create(16, 0)
    b.spawn_random(seed)
    w, shapes = pyoracle.policy_init(9, trained_like=True)
    mask = np.zeros((N, M), np.uint8)
    mask[:, [1, 3]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(12):
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    slot, _ = b.replay_sample(5, 0, batch)
    rows_d, bp_d, bn_d = b.replay_gather_device(slot, batch)
    b.sync()                                                # the gather runs on the handle's stream; raw copies do not wait for it
    n = N * batch
    rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
    assert (rows["ship"] >= 0).all()
    assert (rows["px"] != rows["py"]).any()                  # the transposed index is a different cell
    w_d = DeviceBuffer(w.nbytes).upload(w)
    zeros = np.zeros_like(w)
    m_d, v_d, g_d = DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes)
    l1, l2 = b.dqn_fit_reference(w_d, m_d, v_d, 1, lr, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, gamma, g_d)
    g = g_d.download(np.float32, w.shape).astype(np.float64)

    def maps(buf):
        bits = buf.download(np.uint32, (n, 2, 5000))
        return np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(n, 2, 400, 400)

    xp, xn = maps(bp_d), maps(bn_d)
    t1, t2 = np.zeros((n, 2)), np.zeros((n, 400, 400))
    for s in range(n):
        a_prev, h_prev = R.forward(xp[s, 0], xp[s, 1], rows["head_prev"][s][None], w)
        a_next, h_next = R.forward(xn[s, 0], xn[s, 1], rows["head_next"][s][None], w)
        t1[s], t2[s] = a_prev[0], h_prev[0]
        live = 0.0 if rows["done"][s] else 1.0
        t1[s, int(rows["iaction"][s] != 0)] = rows["reward"][s] + gamma * a_next[0].max() * live
        t2[s, rows["px"][s], rows["py"][s]] = rows["reward"][s] + gamma * h_next[0].max() * live     # [x][y]
    ref = fit_reference(w.astype(np.float64), shapes, xn.astype(np.float64), rows["head_next"], dense=(t1, t2))
    rl1, rl2, rg = ref["l1"], ref["l2"], ref["g"]
    assert abs(l1 - rl1) <= 2e-4 * max(1.0, abs(rl1)) and abs(l2 - rl2) <= 2e-4 * max(1e-9, abs(rl2)) + 1e-12, (l1, rl1, l2, rl2)
    # Every tensor inside 1e-4 of its scale except updense1 (1.25e-3).  tools/fit_precision.py (r03, on the chip)
    # attributes it: the error sits in 7 of the 625 cells of u0 (one cluster; rms 6e-5 of the scale) - one ReLU gate
    # that fp32 and float64 decide differently - not in cancellation noise as r02 guessed: torch's own fp32 autograd on
    # the CPU lands at 1.7e-6 on this minibatch (its rounding leaves that activation on the float64 side).
    compare_gradients(shapes, rg, g, loose=("updense1",))
    b.close()


def test_lean_fit_equals_plain_fit():
    """The two forms of the fit (OFX_OPT_FIT_PLAIN) are the same function: on a minibatch of 24 rows - more tiles per layer
    and several blocks per reduction than the float64 comparisons above afford - every gradient tensor, both losses and
    the batch statistics (through the moved statistics) agree to fp32 summation order, in the textbook and in the
    reference's dense form."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    N, M, seed, batch = 6, 4, 0x0F160077, 4
    b = ArenaBatch(N, M)
    b.replay_create(16, 0)
    b.spawn_random(seed)
    w, shapes = pyoracle.policy_init(5, trained_like=True)
    mask = np.zeros((N, M), np.uint8)
    mask[:, [0, 3]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(10):
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    slot, _ = b.replay_sample(7, 0, batch)
    rows_d, bp_d, bn_d = b.replay_gather_device(slot, batch)
    b.sync()                                                # the gather runs on the handle's stream; raw copies do not wait for it
    n = N * batch
    assert (rows_d.download(b.TRANSITION_DTYPE, (n,))["ship"] >= 0).all()
    rs = np.random.RandomState(3)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    zeros = np.zeros_like(w)
    w_d, m_d, v_d, g_d = (DeviceBuffer(w.nbytes) for _ in range(4))
    out = {}
    # the whole minibatch in both forms of the targets, and its first 1 / 5 rows (one sample: the batch statistics of a
    # single image; an odd count) in the textbook form
    cases = [("textbook", n), ("reference", n), ("textbook", 1), ("textbook", 5)]
    for kind, rows_n in cases:
        for form in ("lean", "plain"):
            b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
            w_d.upload(w); m_d.upload(zeros); v_d.upload(zeros)
            if kind == "textbook":
                l = b.dqn_fit(w_d, m_d, v_d, 1, 1e-4, rows_n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, g_d)
            else:
                l = b.dqn_fit_reference(w_d, m_d, v_d, 1, 1e-4, rows_n, rows_d.ptr, bp_d.ptr, bn_d.ptr, 0.9, g_d)
            out[kind, rows_n, form] = (l, g_d.download(np.float32, w.shape).astype(np.float64), w_d.download(np.float32, w.shape))
    for kind, rows_n in cases:
        (la, ga, wa), (lb, gb, wb) = out[kind, rows_n, "lean"], out[kind, rows_n, "plain"]
        assert np.isfinite(ga).all() and np.abs(ga).max() > 0
        assert abs(la[0] - lb[0]) <= 1e-5 * max(1.0, abs(lb[0])) and abs(la[1] - lb[1]) <= 1e-5 * abs(lb[1]) + 1e-12, (kind, rows_n, la, lb)
        bad = []
        for name, (o, shp) in shapes.items():
            c = int(np.prod(shp))
            layer, what = name.split(".")
            if what in ("mean", "var"):      # moved by the batch statistics of the fit
                np.testing.assert_allclose(wa[o:o + c], wb[o:o + c], rtol=1e-5, atol=1e-7, err_msg="%s %d %s" % (kind, rows_n, name))
                continue
            ko, kshp = shapes[layer + ".kernel"]
            kscale = float(np.abs(gb[ko:ko + int(np.prod(kshp))]).max())
            scale, err = float(np.abs(gb[o:o + c]).max()), float(np.abs(ga[o:o + c] - gb[o:o + c]).max())
            # the two forms round BatchNorm's activation differently (z * scale + shift against gamma * xhat + beta): a
            # ReLU within rounding of zero may be gated differently - the same allowance as against float64
            if err > 1e-4 * scale + 5e-5 * kscale:
                bad.append((name, scale, err))
        assert not bad, (kind, rows_n, bad)
    b.close()


def test_device_trainer_replay_reduces_the_td_error():
    """DeviceTrainer.replay (sample -> gather -> targets -> fit) end to end: repeated fit steps on one minibatch with
    frozen targets drive its own TD error down (a property of the optimiser step, independent of any reference)."""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.trainer import DeviceTrainer
    N, M, seed = 2, 4, 7
    b = ArenaBatch(N, M)
    w, _ = pyoracle.policy_init(4, trained_like=True)
    tr = DeviceTrainer(b, w, learning_rate=1e-3, batch_size=2, memory_size=16)
    b.spawn_random(seed)
    mask = np.zeros((N, M), np.uint8)
    mask[:, 1] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    assert tr.replay() is None                      # empty memories
    for t in range(10):
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    first = tr.replay()
    assert first is not None and np.isfinite(first).all() and tr.fit_steps == 1
    w1 = tr.weights_host()
    assert np.isfinite(w1).all() and np.abs(w1 - w).max() > 0
    # frozen minibatch + frozen targets: the head-1 error must shrink under repeated Adam steps
    slot, _ = b.replay_sample(1, 0, 2)
    rows, bp, bn = b.replay_gather_device(slot, 2)
    n = N * 2
    q_sa, p_sp, y_act, y_ptr = b.dqn_targets(tr.weights.ptr, n, rows.ptr, bp.ptr, bn.ptr, 0.9)
    b.sync()
    ya, yp = DeviceBuffer(4 * n).upload(y_act), DeviceBuffer(4 * n).upload(y_ptr)
    losses = [b.dqn_fit(tr.weights, tr.adam_m, tr.adam_v, tr.fit_steps + 1 + k, 1e-3, n, rows.ptr, bp.ptr, ya.ptr, yp.ptr)
              for k in range(12)]
    assert losses[-1][0] < 0.7 * losses[0][0], losses
    # the reference's step as written, through the same DeviceTrainer.replay
    tr.reference_quirks = True
    steps = tr.fit_steps
    quirky = tr.replay()
    assert np.isfinite(quirky).all() and tr.fit_steps == steps + 1 and np.isfinite(tr.weights_host()).all()
    b.close()


def test_short_memories_are_not_padded_into_the_fit():
    """An arena that holds fewer transitions than the batch size gives -1 pads in ofx_replay_gather (their maps are
    zeroed, not left uninitialised); ofx_replay_gather_valid packs only the real rows - the form Trainer.replay works
    on, batch = min(batch_size, len(memory)) (qlearnIA_V2.py:241-243) - and ofx_dqn_fit refuses a padded batch.  Two
    fits of the packed batch from identical state give the SAME BITS (gradients, updated weights, losses): every
    reduction of the fit combines its partial sums in a fixed order, there is no atomic in it."""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    N, M, seed, bs = 3, 4, 11, 6
    b = ArenaBatch(N, M)
    b.replay_create(16, 0)
    b.spawn_random(seed)
    w, _ = pyoracle.policy_init(2, trained_like=True)
    # arena 0 captures with two ships, arena 1 with one, arena 2 with none: memories of different lengths
    mask = np.zeros((N, M), np.uint8)
    mask[0, [0, 2]] = 1
    mask[1, 1] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(4):
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    cnt, _ = b.replay_count()
    assert cnt[2] == 0 and 0 < cnt[1] < bs and cnt[0] > cnt[1]
    slot, n_s = b.replay_sample(5, 0, bs)
    ns = n_s.download(np.int32, (N,))
    assert list(ns) == [min(int(c), bs) for c in cnt]
    # padded form: pads are ship = -1 rows with EMPTY maps
    rows_h, bp_h, bn_h = b.replay_gather(slot, bs)
    pads = rows_h["ship"] < 0
    assert pads.sum() == N * bs - ns.sum() and pads[2].all()
    assert not bp_h[pads].any() and not bn_h[pads].any()
    # packed form
    total = int(ns.sum())
    rows, bp, bn, got = b.replay_gather_valid(slot, n_s, bs, 0, total)
    assert got == total
    packed = rows.download(b.TRANSITION_DTYPE, (total,))
    assert (packed["ship"] >= 0).all()
    assert np.array_equal(packed, rows_h[~pads])                      # (arena, j) order
    assert np.array_equal(bp.download(np.uint32, (total, 2, 5000)), bp_h[~pads])
    r2, _, _, got2 = b.replay_gather_valid(slot, n_s, bs, 1, 2)       # a window of the packed sequence
    assert got2 == 2 and np.array_equal(r2.download(b.TRANSITION_DTYPE, (2,)), packed[1:3])
    # the fit refuses padding rows ...
    rows_d, bp_d, bn_d = b.replay_gather_device(slot, bs)
    n_all = N * bs
    y = DeviceBuffer(4 * n_all).upload(np.zeros(n_all, np.float32))
    zeros = np.zeros_like(w)
    w_d, m_d, v_d = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(w.nbytes).upload(zeros), DeviceBuffer(w.nbytes).upload(zeros)
    with pytest.raises(Exception, match="padding"):
        b.dqn_fit(w_d, m_d, v_d, 1, 1e-4, n_all, rows_d.ptr, bp_d.ptr, y.ptr, y.ptr)
    assert np.array_equal(w_d.download(np.float32, w.shape), w)       # nothing was updated
    # ... and is deterministic on the packed batch
    grads, news, losses = [], [], []
    for _ in range(2):
        w_d.upload(w); m_d.upload(zeros); v_d.upload(zeros)
        g_d = DeviceBuffer(w.nbytes)
        losses.append(b.dqn_fit(w_d, m_d, v_d, 1, 1e-4, total, rows.ptr, bp.ptr, y.ptr, y.ptr, g_d))
        grads.append(g_d.download(np.float32, w.shape))
        news.append(w_d.download(np.float32, w.shape))
    assert np.isfinite(grads[0]).all() and np.abs(grads[0]).max() > 0
    assert np.array_equal(grads[0], grads[1]) and np.array_equal(news[0], news[1]) and losses[0] == losses[1]
    # the reference's step as written (dense targets: the other loss / seed kernels), twice: the same bits too
    outs = []
    for _ in range(2):
        w_d.upload(w); m_d.upload(zeros); v_d.upload(zeros)
        g_d = DeviceBuffer(w.nbytes)
        l = b.dqn_fit_reference(w_d, m_d, v_d, 1, 1e-4, total, rows.ptr, bp.ptr, bn.ptr, 0.9, g_d)
        outs.append((l, g_d.download(np.float32, w.shape), w_d.download(np.float32, w.shape)))
    assert outs[0][0] == outs[1][0] and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    with pytest.raises(Exception, match="padding"):     # refused before its two predict passes
        b.dqn_fit_reference(w_d, m_d, v_d, 1, 1e-4, n_all, rows_d.ptr, bp_d.ptr, bn_d.ptr, 0.9)
    b.close()


@pytest.mark.parametrize("form", ["lean", "plain"])
def test_adam_recurrence_after_the_first_step(form):
    """Three consecutive ofx_dqn_fit calls (step = 1, 2, 3) on one small minibatch: from the second step on the decay terms
    b1 * m and b2 * v and the bias correction of t_adam (ofx_train.hip) carry values a step-1 comparison from zero moments
    cannot tell apart.  After every step the recurrence is evaluated in float64 from the device's OWN gradient and the
    previous device m, v, w:
        m = 0.9 m + 0.1 g      v = 0.999 v + 0.001 g^2      w -= lr sqrt(1 - 0.999^t) / (1 - 0.9^t) m / (sqrt(v) + 1e-7)
    m and v are two fp32 products and a sum with rounded constants: 8 * 2^-24 of the sum of the two terms' magnitudes.
    w: the allowance of the step-1 check of test_dqn_fit_vs_torch_autograd.  The moving BatchNorm statistics are not
    Adam's (excluded, as there)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    b, n, rows_d, bp_d, bn_d = collect_minibatch(3)
    b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
    w0, shapes = pyoracle.policy_init(9, trained_like=True)
    rs = np.random.RandomState(5)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    zeros = np.zeros_like(w0)
    w_d, m_d, v_d, g_d = (DeviceBuffer(w0.nbytes) for _ in range(4))
    w_d.upload(w0); m_d.upload(zeros); v_d.upload(zeros)
    lr, ulp = 1e-3, 8 * 2.0 ** -24
    w, m, v = (a.astype(np.float64) for a in (w0, zeros, zeros))
    for t in (1, 2, 3):
        loss = b.dqn_fit(w_d, m_d, v_d, t, lr, n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, g_d)
        assert np.isfinite(loss).all()
        g = g_d.download(np.float32, w0.shape).astype(np.float64)
        w1, m1, v1 = (buf.download(np.float32, w0.shape).astype(np.float64) for buf in (w_d, m_d, v_d))
        m_ref, v_ref = 0.9 * m + 0.1 * g, 0.999 * v + 0.001 * g * g
        w_ref = w - lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t) * m_ref / (np.sqrt(v_ref) + 1e-7)
        # (+ 2^-148: below 2^-126 fp32 rounds to a fixed spacing of 2^-149, not to 2^-24 of the value - g * g underflows
        # for the smallest gradients - and each of the three operations may lose half of that spacing)
        m_tol = ulp * (np.abs(0.9 * m) + np.abs(0.1 * g)) + 2.0 ** -148
        v_tol = ulp * (0.999 * v + 0.001 * g * g) + 2.0 ** -148
        for name, (o, shp) in shapes.items():
            c = int(np.prod(shp))
            if name.split(".")[1] in ("mean", "var"):
                continue
            s = slice(o, o + c)
            em = float((np.abs(m1[s] - m_ref[s]) / m_tol[s]).max())          # worst error, in units of its bound
            ev = float((np.abs(v1[s] - v_ref[s]) / v_tol[s]).max())
            ew = float(np.abs(w1[s] - w_ref[s]).max())
            print("step %d %-5s %-18s m %.3f of its bound, v %.3f of its bound, w err %.2e" % (t, form, name, em, ev, ew))
            assert em <= 1.0, (t, name, "adam_m: worst error, in bounds", em)
            assert ev <= 1.0, (t, name, "adam_v: worst error, in bounds", ev)
            assert ew <= 2e-7 + 1e-6 * float(np.abs(w[s]).max()), (t, name, "w", ew)
        assert np.abs(g).max() > 0
        if t > 1:                                # the decay terms are there: the moments are not a function of g alone
            assert np.abs(m).max() > 0 and np.abs(v).max() > 0
        w, m, v = w1, m1, v1
    b.close()


# ---- the lean fit in the regime it is USED in (r04): minibatches of 128 - 4096 rows -------------------------------
# Every persistent kernel of ofx_fit.hip loops over several tiles per block there (OFX_FIT_MAX_BLOCKS = 2048, 1024 for
# the weight-gradient kernels), the reductions go through their two-level ordered combines and f_bits_corr through its
# per-block partial rows - paths the 4- and 24-row comparisons above reach with one tile per block only.

@pytest.mark.parametrize("rows,skip", [(128, 0), (1024, 4), (1024, 0)])
def test_lean_fit_equals_plain_fit_large_batches(rows, skip):
    """lean == plain at 128 rows (every persistent kernel past its first tile: f_conv_fwd at 200x200 loops from 52 rows,
    f_b1_pool / f_b1_up / f_first_bwd / f_bits_corr from 26 - 205) and at 1024 rows (the bench's regime; the
    plain form holds 62 GB of workspace there), textbook and reference targets: the per-tensor bounds of
    test_lean_fit_equals_plain_fit, equal moved statistics, and two lean runs give the same bits.

    (1024, 0) - rows 0 .. 1023 of the collection - is the one minibatch found in r04 on which the two forms differ by more
    than fp32 summation order in the textbook form.  It is THAT set of rows, not the size: every window of the same
    collection shifted by 1, 4, 512, 1000 or 1024 rows, every prefix up to 1023 and the 2048-row batch agree to <= 1e-4
    (tools/fit_bisect.py, profiles/r04_fit_bisect.txt).  Five tensors get 2e-3 on that case: conv1.kernel, conv1.gamma,
    conv1.beta, conv2.kernel and conv2.beta; everything else and (1024, 4) keep the strict bound.
    What is measured about it (tests/test_gpu_fit_fp64_1024.py, profiles/r16_fit_fp64.txt): against float64 the plain form
    meets the strict bounds there and the LEAN form carries the difference (4.5e-4 / 1.1e-3 / 6.8e-4 of scale on
    conv1.kernel / conv1.gamma / conv2.kernel); torch's own float32 autograd of the graph, which has nothing of
    f_first_bwd's decomposition, shows the same figures and lies within 3e-6 of scale of the lean form on those three.  That
    rules out a defect of the decomposition.  A dense ReLU gate and fp32 rounding of the batch statistics or of
    BatchNorm-backward's per-channel sums are ruled out as well (float64 with those forced or rounded stays with float64;
    carrying the coefficients as float pairs in the kernel had changed nothing either).  The cause is OPEN between a
    decision inside the trunk (a ReLU gate, a max-pool arg-max) that the plain form takes as float64 does and the other two
    do not, and element-wise fp32 rounding that does not average out: no margin and no forced evaluation shows which."""
    from ofighters_amd import DeviceBuffer, _native as nat
    b, n_all, rows_all, bp_all, bn_all = collect_minibatch((rows + skip + 3) // 4)
    n = rows
    assert n_all >= n + skip

    class _Off:                     # the window [skip, skip + rows) of the gathered minibatch
        def __init__(self, buf, stride): self.ptr = buf.ptr + skip * stride
    rows_d, bp_d, bn_d = _Off(rows_all, b.TRANSITION_DTYPE.itemsize), _Off(bp_all, 40000), _Off(bn_all, 40000)
    loose = {"conv1.kernel", "conv1.gamma", "conv1.beta", "conv2.kernel", "conv2.beta"} if (rows, skip) == (1024, 0) else set()
    check_lean_equals_plain(b, n, rows_d, bp_d, bn_d, loose)
    b.close()


@pytest.mark.parametrize("case", ["dense", "half", "full", "frame"])
def test_lean_fit_on_maps_without_empty_windows(case):
    """The first layer's backward (f_first_bwd) visits only the 2 x 2 windows that see a set bit and takes the empty ones'
    share from border sums of the second layer's dz.  Arena observations leave ~97 % of the windows empty; here NONE is
    (30 % of the cells set; 60 % and 50 %), one half of the plane is and the other is not (the border
    terms with both kinds of window on the frame), or only the plane's frame is set - same bounds against the plain form."""
    b, n, rows_d, bp_d, bn_d = collect_minibatch(3)
    rs = np.random.RandomState(11)
    for buf in (bp_d, bn_d):
        x = np.zeros((n, 2, 400, 400), bool)
        if case == "dense":
            x[:, 0] = rs.uniform(size=(n, 400, 400)) < 0.3
            x[:, 1] = rs.uniform(size=(n, 400, 400)) < 0.05
        elif case == "half":
            x[:, 0, :, :200] = rs.uniform(size=(n, 400, 200)) < 0.3
            x[:, 1, 200:, :] = rs.uniform(size=(n, 200, 400)) < 0.02
        elif case == "full":      # (every cell of a map set is degenerate: one table entry for 158 404 pixels of a plane,
            x[:, 0] = rs.uniform(size=(n, 400, 400)) < 0.6     # every pooling window a four-way tie - both forms resolve it,
            x[:, 1] = rs.uniform(size=(n, 400, 400)) < 0.5     # not the same way: conv2's own gradient moves by 1e-3 there)
        else:
            x[:, 0, [0, 399], :] = True
            x[:, 0, :, [0, 399]] = True
            x[:, 1, 100:300, 100:300] = rs.uniform(size=(n, 200, 200)) < 0.01
        buf.upload(np.packbits(x.reshape(n, 2, 160000), axis=-1, bitorder="little").view(np.uint32))
    # updense1: one ReLU gate of u0 that the two forms may decide differently on synthetic maps (the allowance of the float64
    # comparisons above, tools/fit_precision.py) - this test is about the trunk's first layers
    check_lean_equals_plain(b, n, rows_d, bp_d, bn_d, loose_both={"updense1.kernel", "updense1.bias"})
    b.close()


def test_lean_fit_at_4096_rows(tmp_path):
    """The bench's fit_batch: 4096 rows, lean form.  Two runs give the same bits, everything is finite, and the moved
    statistics of EVERY BatchNorm - conv1 first (the layer the lean fit never materialises: its statistics come from the
    autocorrelation of the 1-bit maps) up to upconv3 (the last normalised layer, behind all others) - equal
    0.99 * old + 0.01 * (batch mean | biased batch variance) of a float64 evaluation of the same minibatch."""
    from ofighters_amd import DeviceBuffer, _native as nat
    b, n, rows_d, bp_d, bn_d = collect_minibatch(1024)
    assert n == 4096
    w, shapes = pyoracle.policy_init(5, trained_like=True)
    rs = np.random.RandomState(3)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    bufs = tuple(DeviceBuffer(w.nbytes) for _ in range(4))
    b.set_option(nat.OPT_FIT_PLAIN, 0)
    for kind in ("textbook", "reference"):
        la, ga, wa = fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs)
        la2, ga2, wa2 = fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs)
        assert la == la2 and np.array_equal(ga, ga2) and np.array_equal(wa, wa2), kind
        assert np.isfinite(ga).all() and np.isfinite(wa).all() and np.isfinite(la).all() and np.abs(ga).max() > 0
        rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
        bits = (bn_d if kind == "reference" else bp_d).download(np.uint32, (n, 2, 5000))     # the reference fits on next_state
        vec8 = rows["head_next" if kind == "reference" else "head_prev"]
        stats = batch_statistics_f64(tmp_path, w.astype(np.float64), shapes, bits, vec8)
        for layer, (bm, bv) in stats.items():
            for what, batch_stat in (("mean", bm), ("var", bv)):
                o, shp = shapes[layer + "." + what]
                c = int(np.prod(shp))
                want = 0.99 * w[o:o + c].astype(np.float64) + 0.01 * batch_stat
                moved = wa[o:o + c].astype(np.float64) - 0.99 * w[o:o + c]
                # the comparison is on the 1 % that moved: (new - 0.99 old) / 0.01 against the float64 batch statistic
                scale = max(float(np.abs(batch_stat).max()), 1e-6)
                err = float(np.abs(moved / 0.01 - batch_stat).max())
                print("%-10s %-8s %-4s batch statistic scale %.3e  err %.2e" % (kind, layer, what, scale, err))
                assert err <= 2e-4 * scale + 2e-5, (kind, layer, what, err, scale)
                np.testing.assert_allclose(wa[o:o + c], want, rtol=5e-6, atol=1e-6)
    b.close()


def test_one_handle_relays_its_blocks_for_every_form():
    """Every hand-carved workspace is one layout run twice (ofx_arena.h): measured, then laid out on the handle's block.  A
    block that was sized, grown, given back and laid out again for another form leaves nothing behind that a later call can
    see.  ONE handle runs, in this order: a lean fit of 2 rows, a plain fit of 16, the lean fit again, Double-DQN targets on
    5 rows, a sampling forward, a plain forward, the lean fit a third time.  The three lean fits start from the same weights
    and return the same bits (losses, gradient, weights, moments); the targets and both forwards equal, bit for bit, the
    same calls made first on a fresh handle in the same state.

    The give-back rule fires on the way: by the layouts' per-row counts a lean row is 9.3 MB and a plain row 36.9 MB, so
    the 16-row plain block holds 590 MB of rows, while the 2-row lean block is 19 MB of rows plus under 20 MB of buffers
    that do not grow with the rows (the 9.6 MB of block partials, the correlation rows, the gradient, dense1 transposed) -
    less than a quarter of the plain block: the second lean fit frees the block and allocates its own size anew."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    N, M, seed, batch = 2, 2, 0x0F160077, 8
    S, n = N * M, N * batch
    w, _ = pyoracle.policy_init(5, trained_like=True)
    w2, _ = pyoracle.policy_init(6, trained_like=True)
    rs = np.random.RandomState(3)
    y_h, y2_h = rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)
    zeros = np.zeros_like(w)

    class Rig:
        def __init__(self):
            b = self.b = ArenaBatch(N, M)
            b.replay_create(16, 0)
            b.spawn_random(seed)
            mask_d = DeviceBuffer(S).upload(np.ones((N, M), np.uint8))
            ia_d, ip_d = DeviceBuffer(4 * S), DeviceBuffer(8 * S)
            for t in range(10):
                b.bot_actions(["random"] * M, seed, tick=t)
                b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
                b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
                b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
                b.step(actions_ptr=b._actions.ptr)
            slot, _ = b.replay_sample(7, 0, batch)
            self.rows_d, self.bp_d, self.bn_d = b.replay_gather_device(slot, batch)
            b.sync()                                        # the gather runs on the handle's stream; raw copies do not wait for it
            assert (self.rows_d.download(b.TRANSITION_DTYPE, (n,))["ship"] >= 0).all()
            self.y, self.y2 = DeviceBuffer(4 * n).upload(y_h), DeviceBuffer(4 * n).upload(y2_h)
            self.bufs = tuple(DeviceBuffer(w.nbytes) for _ in range(4))
            self.online, self.target = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(w2.nbytes).upload(w2)

        def fit(self, plain, rows_n):
            w_d, m_d, v_d, g_d = self.bufs
            self.b.set_option(nat.OPT_FIT_PLAIN, int(plain))
            w_d.upload(w); m_d.upload(zeros); v_d.upload(zeros)
            l = self.b.dqn_fit(w_d, m_d, v_d, 1, 1e-4, rows_n, self.rows_d.ptr, self.bp_d.ptr, self.y.ptr, self.y2.ptr, g_d)
            return [np.array(l)] + [d.download(np.float32, w.shape) for d in (g_d, w_d, m_d, v_d)]

        def targets(self):
            outs = [DeviceBuffer(4 * 5) for _ in range(4)]    # q_sa, p_sp, y_act, y_ptr
            self.b.dqn_targets_double_into(self.online.ptr, self.target.ptr, 5, self.rows_d.ptr, self.bp_d.ptr, self.bn_d.ptr, 0.9,
                                           outs[2].ptr, outs[3].ptr, q_sa_ptr=outs[0].ptr, p_sp_ptr=outs[1].ptr)
            self.b.sync()
            return [o.download(np.float32, (5,)) for o in outs]

        def boltzmann(self):
            vals = [DeviceBuffer(4 * S) for _ in range(4)]
            self.b.policy_act_boltzmann(self.online.ptr, 0.5, 0.7, 1.3, seed, tick=3, q_sa_ptr=vals[0].ptr, p_sp_ptr=vals[1].ptr,
                                        v_act_ptr=vals[2].ptr, v_ptr_ptr=vals[3].ptr)
            self.b.policy_actions()                            # the handle's kept (iaction, ipointer), as packed actions
            acts = self.b.actions_host()
            return [v.download(np.float32, (S,)) for v in vals] + [np.ascontiguousarray(acts[k]) for k in ("valid", "shoot", "thrust", "px", "py")]

        def forward(self):
            act_d, ia_d, ip_d, heat_d = DeviceBuffer(8 * S), DeviceBuffer(4 * S), DeviceBuffer(8 * S), DeviceBuffer(4 * S * 160000)
            self.b.policy_forward(self.target.ptr, None, act_d.ptr, ia_d.ptr, ip_d.ptr, heat_d.ptr)
            self.b.sync()
            return [act_d.download(np.float32, (S, 2)), ia_d.download(np.int32, (S,)), ip_d.download(np.int32, (S, 2)),
                    heat_d.download(np.float32, (S, 160000))]

    def same(a, c):
        return len(a) == len(c) and all(x.dtype == z.dtype and np.array_equal(x.view(np.uint8), z.view(np.uint8)) for x, z in zip(a, c))

    fresh = Rig()
    want_targets, want_boltzmann, want_forward = fresh.targets(), fresh.boltzmann(), fresh.forward()
    fresh.b.close()
    assert all(np.isfinite(x).all() for x in want_targets + want_forward[:1])

    one = Rig()
    lean1 = one.fit(False, 2)
    plain = one.fit(True, 16)
    lean2 = one.fit(False, 2)
    got_targets, got_boltzmann, got_forward = one.targets(), one.boltzmann(), one.forward()
    lean3 = one.fit(False, 2)
    one.b.close()
    assert np.isfinite(lean1[1]).all() and np.abs(lean1[1]).max() > 0 and np.isfinite(plain[1]).all()
    assert same(lean1, lean2), "the lean fit behind a 16-row plain fit"
    assert same(lean1, lean3), "the lean fit behind the targets and the forwards"
    assert same(want_targets, got_targets), "ofx_dqn_targets_double behind the fits"
    assert same(want_boltzmann, got_boltzmann), "ofx_policy_act_boltzmann behind the fits"
    assert same(want_forward, got_forward), "ofx_policy_forward behind the fits"
