"""The DQN fit at 256 rows - the default fit_batch, above every multi-tile threshold of ofx_fit.hip (26 - 205 rows, see the
comment above tests/test_train.py::test_lean_fit_equals_plain_fit_large_batches) - against a float64 evaluation of the declared graph:
tests/fit_ref64.py, the chunked checker, in ONE child process for the whole module (torch on the GPU; it shares nothing
with libofx).  The module's fixture runs every fit, downloads what the tests compare, closes the handle and then spawns
the child; the tests only compare.

Rows: collect_minibatch(64); weights policy_init(5, trained_like=True); targets RandomState(3) - the inputs of
tests/fit_cases.py::check_lean_equals_plain.

Bounds - all the project's own:
    losses                      rel 1e-4                                   (test_dqn_fit_vs_torch_autograd)
    every gradient tensor       err <= 1e-4 scale + 5e-5 kscale            (compare_gradients; its structure rule for the
                                                                            tensors the 4-row float64 tests pass as loose:
                                                                            updense1 under dense targets)
    bias in front of BatchNorm  <= 2e-4 kscale (its true gradient is zero) (check_lean_equals_plain)
    moved statistics            the rule of test_lean_fit_at_4096_rows against the checker's batch statistics
    Adam step 1                 from the device's own gradient, as in test_dqn_fit_vs_torch_autograd
    td [n][2]                   no project bound: 4 x the error of the float32 yardstick on the per-row errors
The child also evaluates every case in float32 - what plain fp32 rounding does to this graph at this size, the
yardstick - and every figure goes to fit_fp64_report.json in the report folder of tests/policy_fp64_cases.py
(profiles/r16_fit_fp64.txt is a copy)."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.fit_fp64_cases import (LR, check_gradient, check_losses, check_update, fit_buffers, report as _report, report_case,
                                  reset_buffers, run_checker)

pytestmark = pytest.mark.gpu

DELTA = 0.5
ROBUST_DRAW = 1        # which pair of RandomState(3)'s draws gives the robust case its targets (see the fixture)
BN_LAYERS = ("conv1", "conv2", "conv3", "conv4", "upconv1", "upconv2", "upconv3")


def clear_of_delta(e):
    """no error within 1e-3 delta of delta (the guard of test_robust_lean_fit_equals_plain_fit_at_128_rows)"""
    return bool((np.abs(np.abs(e.astype(np.float64)) / DELTA - 1.0) >= 1e-3).all())


# -------------------------------------------------------------------------------------------------- the fixture
@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    from ofighters_amd import DeviceBuffer, _native as nat
    from tests.fit_cases import collect_minibatch
    b, n, rows_d, bp_d, bn_d = collect_minibatch(64)
    assert n == 256
    w, shapes = pyoracle.policy_init(5, trained_like=True)
    rs = np.random.RandomState(3)
    y_act, y_ptr = rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)
    row_w = np.random.RandomState(6).uniform(0.05, 1.0, n).astype(np.float32)
    y, y2, rw_d, td_d = (DeviceBuffer(4 * n).upload(y_act), DeviceBuffer(4 * n).upload(y_ptr), DeviceBuffer(4 * n).upload(row_w),
                         DeviceBuffer(8 * n))
    bufs = fit_buffers(w)
    w_d, m_d, v_d, g_d = bufs

    def result(l):
        return dict(loss=l[:2], g=g_d.download(np.float32, w.shape), w_new=w_d.download(np.float32, w.shape))

    out = {}
    for legacy in (0, 1):
        b.set_option(nat.OPT_BILINEAR_LEGACY, legacy)
        for form in ("lean", "plain"):
            b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
            reset_buffers(bufs, w)
            out["textbook_legacy" if legacy else "textbook", form] = result(
                b.dqn_fit(w_d, m_d, v_d, 1, LR, n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, g_d))
    b.set_option(nat.OPT_BILINEAR_LEGACY, 0)
    b.set_option(nat.OPT_FIT_PLAIN, 0)
    reset_buffers(bufs, w)
    out["reference", "lean"] = result(b.dqn_fit_reference(w_d, m_d, v_d, 1, LR, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, 0.9, g_d))
    # The robust case rejects targets that put any error within 1e-3 delta of delta (there the fit and the checker could
    # put a row in different zones).  The textbook targets above - pair 0 of RandomState(3)'s stream - do that at 256 rows
    # (with 512 errors spread over a few delta about one pair in six does), so the case is FIXED on pair ROBUST_DRAW = 1 of
    # the same stream (nearest |e| / delta 1.0016).  The test asserts the guard on the fit's and on the checker's errors.
    for _ in range(ROBUST_DRAW):
        y_act_r, y_ptr_r = rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)
    yr, y2r = DeviceBuffer(4 * n).upload(y_act_r), DeviceBuffer(4 * n).upload(y_ptr_r)
    reset_buffers(bufs, w)
    robust = result(b.dqn_fit_robust(w_d, m_d, v_d, 1, LR, n, rows_d.ptr, bp_d.ptr, yr.ptr, y2r.ptr, DELTA, 0.0,
                                     row_weight_ptr=rw_d.ptr, td_ptr=td_d.ptr, grad_buf=g_d))
    b.sync()
    robust["td"], robust["draw"] = td_d.download(np.float32, (n, 2)), ROBUST_DRAW
    out["robust", "lean"] = robust
    reset_buffers(bufs, w)
    acc = DeviceBuffer(4 * b.dqn_acc_floats())
    b.dqn_grad(w_d, n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, acc, True)
    l = b.dqn_apply(w_d, m_d, v_d, 1, LR, acc, scale=1.0)
    b.sync()
    out["grad_apply", "lean"] = dict(loss=l[:2], g=acc.download(np.float32, (b.dqn_acc_floats(),))[:w.size],
                                     w_new=w_d.download(np.float32, w.shape))
    rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
    arrays = dict(bits_prev=bp_d.download(np.uint32, (n, 2, 5000)), bits_next=bn_d.download(np.uint32, (n, 2, 5000)),
                  head_prev=np.ascontiguousarray(rows["head_prev"]), head_next=np.ascontiguousarray(rows["head_next"]),
                  iaction=rows["iaction"].astype(np.int64), px=rows["px"].astype(np.int64), py=rows["py"].astype(np.int64),
                  reward=rows["reward"].astype(np.float64), done=(rows["done"] != 0).astype(np.uint8), y_act=y_act, y_ptr=y_ptr,
                  row_w=row_w, y_act_robust=y_act_r, y_ptr_robust=y_ptr_r)
    b.close()                                         # the child has the card to itself
    text = dict(bits="bits_prev", vec8="head_prev", iaction="iaction", px="px", py="py", y_act="y_act", y_ptr="y_ptr",
                dtypes=["float64", "float32"], chunk=32)
    cases = [dict(name="textbook", **text), dict(name="textbook_legacy", legacy=True, **text),
             dict(name="robust", row_w="row_w", huber_delta=DELTA, **dict(text, y_act="y_act_robust", y_ptr="y_ptr_robust")),
             dict(name="reference", bits="bits_next", vec8="head_next", iaction="iaction", px="px", py="py",
                  replay=dict(bits_prev="bits_prev", vec8_prev="head_prev", reward="reward", done="done", gamma=0.9),
                  dtypes=["float64", "float32"], chunk=32)]
    ref, seconds = run_checker(tmp_path_factory.mktemp("fit64"), w, shapes, cases, arrays, timeout=900)
    _report("256_rows_checker", dict(child_seconds=seconds, cases=len(cases), rows=n, chunk=32))
    return dict(w=w, shapes=shapes, n=n, out=out, ref=ref)


# WIDENED[case][tensor] = the bound's factor on scale where the float32 yardstick itself exceeds half the project's bound
# (then 4 x the yardstick, the figure from profiles/r16_fit_fp64.txt).  Empty: no tensor needed it.
WIDENED = {}


def _check_case(fits, case, forms, loose_layers=()):
    s, res = fits["shapes"], fits["ref"][case]
    report_case("256_rows_" + case, s, res, {f: fits["out"][case, f]["g"] for f in forms})
    bad = []
    for form in forms:
        o = fits["out"][case, form]
        assert np.isfinite(o["g"]).all() and np.abs(o["g"]).max() > 0
        check_losses(o["loss"], res["float64"]["loss"])
        bad += [(form,) + m for m in check_gradient("%s %s" % (case, form), s, res["float64"]["g"], o["g"], loose_layers,
                                                    widened=WIDENED.get(case))]
        check_update(s, fits["w"], o["g"], o["w_new"], res["float64"]["stats"])
    check_gradient("%s fp32 yardstick" % case, s, res["float64"]["g"], res["float32"]["g"], loose_layers)
    assert not bad, (case, bad)


@pytest.mark.parametrize("legacy", [False, True])
def test_textbook_fit_at_256_rows(fits, legacy):
    """lean and plain form, half-pixel and legacy bilinear (f_b1_up's closed-form up-sampling coefficients cross tile
    boundaries only at sizes like this one)"""
    _check_case(fits, "textbook_legacy" if legacy else "textbook", ("lean", "plain"))
    a, c = fits["out"]["textbook", "lean"]["g"], fits["out"]["textbook_legacy", "lean"]["g"]
    assert not np.array_equal(a, c)                  # the option reached the fit


def test_reference_fit_at_256_rows(fits):
    """ofx_dqn_fit_reference: dense targets (the float64 inference-mode predictions with Trainer.replay's two entries
    replaced, fit_ref64.dense_targets), fitted on bits_next / head_next.  updense1: the structure rule of
    test_dqn_fit_reference_quirks."""
    _check_case(fits, "reference", ("lean",), loose_layers=("updense1",))


def test_robust_fit_at_256_rows(fits):
    """ofx_dqn_fit_robust with random row weights and huber_delta = 0.5, no clip; the returned td [n][2] against the
    checker's per-row errors.  No error may lie within 1e-3 delta of delta (the guard of
    test_robust_lean_fit_equals_plain_fit_at_128_rows): there the fit and the checker could put a row in different zones.
    The textbook targets trip that guard at 256 rows, so the case has its own fixed pair of draws; the guard is asserted here."""
    res, td = fits["ref"]["robust"], fits["out"]["robust", "lean"]["td"].astype(np.float64)
    e64, e32 = res["float64"]["e"], res["float32"]["e"]
    for e in (td, e64):
        r = np.abs(e) / DELTA
        print("draw %d of the targets; nearest |e| / delta to 1: %.6f; errors beyond delta: %d of %d"
              % (fits["out"]["robust", "lean"]["draw"], r.ravel()[np.abs(r - 1).argmin()], (r > 1).sum(), r.size))
        assert clear_of_delta(e), "an error within 1e-3 delta of delta: the case is not a valid one"
        assert (r > 1).any() and (r < 1).any()
    rec = {"targets": "draw %d of RandomState(3)'s pairs" % fits["out"]["robust", "lean"]["draw"]}
    heads = ("e1", "e2")
    for k, head in enumerate(heads):
        yard, err = float(np.abs(e32[:, k] - e64[:, k]).max()), float(np.abs(td[:, k] - e64[:, k]).max())
        rec[head] = dict(scale=float(np.abs(e64[:, k]).max()), lean=err, fp32=yard)
        print("td %s: scale %.3e  lean %.3e  fp32 yardstick %.3e" % (head, rec[head]["scale"], err, yard))
    _report("256_rows_robust_td", rec)
    _check_case(fits, "robust", ("lean",))
    for head in heads:
        assert rec[head]["lean"] <= 4 * rec[head]["fp32"], (head, rec[head])


def test_grad_then_apply_is_the_fused_fit_at_256_rows(fits):
    """ofx_dqn_grad(reset = 1) + ofx_dqn_apply(scale = 1) on the same rows: the bits of the fused textbook fit - gradient,
    losses, new blob - so the float64 comparison of the textbook case holds for it as it stands"""
    a, f = fits["out"]["grad_apply", "lean"], fits["out"]["textbook", "lean"]
    assert tuple(a["loss"]) == tuple(f["loss"])
    assert np.array_equal(a["g"], f["g"]) and np.array_equal(a["w_new"], f["w_new"])
