"""The textbook fit at 1024 rows against the chunked float64 checker (tests/fit_ref64.py on the GPU, one child for the
module), on the two windows of tests/test_train.py::test_lean_fit_equals_plain_fit_large_batches:

    window 0   rows [0, 1024) of collect_minibatch(256) - the minibatch on which the lean form sits 4.5e-4 / 1.1e-3 /
               6.8e-4 of scale away from float64 on conv1.kernel / conv1.gamma / conv2.kernel
    control    rows [4, 1028) of collect_minibatch(257)

The bounds are those of tests/test_gpu_fit_fp64.py, strict on every tensor, against float64 - with ONE freedom, shown
and not assumed: a ReLU gate of dense1 / dense2 / updense1 that is a near-tie may be decided either way.  The child
evaluates every window in float64, in float32 (the yardstick: torch's own float32 autograd of the graph) and in float64
with the near-tie dense gates forced the float32 way (fit_ref64.near_tie_gates: the two evaluations decide the gate
differently AND its float64 margin is below twice the largest deviation of that layer's float32 pre-activations).  A form
passes a window if it meets the strict bounds against one of the two float64 evaluations; a gate that differs without
being a near-tie fails the test.  Measured (profiles/r16_fit_fp64.txt):

    control    against plain float64 lean, plain and the yardstick ALL sit 1e-3 .. 2.7e-3 of scale away on twelve tensors of
               the trunk and dense2.  There is exactly one near-tie: dense2's unit 44 on row 443 (float64 +1.1e-6, float32
               -1.1e-5).  With that one gate forced, all three meet the strict bounds on every tensor.
    window 0   one near-tie, updense1's unit 489 on row 589: it accounts for the yardstick's updense1.kernel (4.9e-4) and
               for nothing else; both forms decide it as float64 does.  The five tensors conv1.kernel / gamma / beta,
               conv2.kernel / beta of the LEAN form stay on the project's existing 2e-3 allowance against float64 - and
               are held to the strict bound against the YARDSTICK, which sits where the lean form sits (4.53e-4 / 1.13e-3 /
               6.78e-4 against lean 4.50e-4 / 1.13e-3 / 6.78e-4; apart by 2.8e-6 / 1.7e-6 / 7.0e-5 / 1.4e-6 / 1.6e-4).

What that settles about the five tensors, and what it does not.  Ruled out: a defect of f_first_bwd's decomposition (an
evaluation with no K1 + delta split, border sums or sum(dz) = 0 gives the lean gradient); a dense ReLU gate; fp32 rounding
of the forward batch statistics and of the per-channel sums of BatchNorm's backward (float64 with either rounded to
float32 stays with float64: the report's fp32stats / fp32coef columns).  OPEN: a decision inside the trunk (a ReLU gate
or a max-pool arg-max that float32 autograd and the lean form take one way, float64 and the plain form the other) against
element-wise fp32 rounding that does not average out.  No trunk margin and no forced trunk evaluation is shown."""
import numpy as np
import pytest

from oracle import pyoracle
from tests.fit_fp64_cases import (LR, check_gradient, check_losses, check_update, fit_buffers, report as _report, report_case,
                                  reset_buffers, run_checker, tensor_errors)

pytestmark = pytest.mark.gpu

DENSE = ("dense1", "dense2", "updense1")
FIVE = ("conv1.kernel", "conv1.gamma", "conv1.beta", "conv2.kernel", "conv2.beta")
WINDOWS = {"window0": (256, 0), "control": (257, 4)}
ROWS, CHUNK = 1024, 32


def fit_both_windows(tmp):
    """both forms on both windows, then - the handles closed - the checker on both: one child"""
    from ofighters_amd import DeviceBuffer, _native as nat
    from tests.fit_cases import collect_minibatch
    w, shapes = pyoracle.policy_init(5, trained_like=True)
    rs = np.random.RandomState(3)
    y_act, y_ptr = rs.uniform(-1, 2, ROWS).astype(np.float32), rs.uniform(-1, 2, ROWS).astype(np.float32)
    out, arrays, cases, workspace = {}, dict(y_act=y_act, y_ptr=y_ptr), [], {}
    for name, (arenas, skip) in WINDOWS.items():
        b, n_all, rows_all, bp_all, bn_all = collect_minibatch(arenas)
        assert n_all >= ROWS + skip
        y, y2 = DeviceBuffer(4 * ROWS).upload(y_act), DeviceBuffer(4 * ROWS).upload(y_ptr)
        bufs = fit_buffers(w)
        w_d, m_d, v_d, g_d = bufs
        for form in ("lean", "plain"):
            b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
            reset_buffers(bufs, w)
            l = b.dqn_fit(w_d, m_d, v_d, 1, LR, ROWS, rows_all.ptr + skip * b.TRANSITION_DTYPE.itemsize, bp_all.ptr + skip * 40000,
                          y.ptr, y2.ptr, g_d)
            out[name, form] = dict(loss=l, g=g_d.download(np.float32, w.shape), w_new=w_d.download(np.float32, w.shape))
        rows = rows_all.download(b.TRANSITION_DTYPE, (n_all,))[skip:skip + ROWS]
        arrays.update({name + "_bits": bp_all.download(np.uint32, (n_all, 2, 5000))[skip:skip + ROWS],
                       name + "_vec8": np.ascontiguousarray(rows["head_prev"]), name + "_ia": rows["iaction"].astype(np.int64),
                       name + "_px": rows["px"].astype(np.int64), name + "_py": rows["py"].astype(np.int64)})
        cases.append(dict(name=name, bits=name + "_bits", vec8=name + "_vec8", iaction=name + "_ia", px=name + "_px",
                          py=name + "_py", y_act="y_act", y_ptr="y_ptr", dtypes=["float64", "float32"],
                          variants=["fp32gates"] + (["fp32stats", "fp32coef"] if name == "window0" else []), chunk=CHUNK))
        b.close()                                     # the plain form's 62 GB go back before the child starts
    ref, seconds = run_checker(tmp, w, shapes, cases, arrays, timeout=1100)
    peak = max(float(ref[c][dt]["peak_bytes"]) for c in ref for dt in ref[c]) / 2 ** 30
    _report("1024_rows_checker", dict(child_seconds=seconds, cases=len(cases), rows=ROWS, chunk=CHUNK, peak_gb=peak))
    assert peak < 62.0          # below the fit's own workspace at this size (the plain form's)
    return dict(w=w, shapes=shapes, out=out, ref=ref)


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    return fit_both_windows(tmp_path_factory.mktemp("fit64"))


@pytest.mark.parametrize("window,form", [("window0", "plain"), ("control", "plain"), ("control", "lean"), ("window0", "lean")])
def test_textbook_fit_at_1024_rows(fits, window, form):
    s, res, o = fits["shapes"], fits["ref"][window], fits["out"][window, form]
    lean = fits["out"][window, "lean"]["g"]
    apart = tensor_errors(s, res["float32"]["g"], lean)
    forced = res["float64_fp32gates"]
    ties = {layer: forced["forced_" + layer].tolist() for layer in DENSE}
    extra = dict(_near_tie_dense_gates=ties, _lean_minus_fp32={name: apart[name][2] for name in FIVE},
                 _min_abs_preactivation={layer: float(res["float64"]["minpre_" + layer].min()) for layer in DENSE},
                 _five_tensors="window0, lean: 2e-3 of scale against float64, strict against the float32 yardstick; ruled "
                               "out: f_first_bwd's decomposition, dense gates, fp32 statistics and BatchNorm-backward sums; "
                               "open: a trunk decision or element-wise fp32 rounding")
    for key in res:                                   # every float64 variant as a column of its own, against plain float64
        if key.startswith("float64_"):
            extra["_variant_" + key] = {name: v[2] for name, v in tensor_errors(s, res["float64"]["g"], res[key]["g"]).items()}
            extra["_lean_minus_" + key] = {name: v[2] for name, v in tensor_errors(s, res[key]["g"], lean).items() if name in FIVE}
    report_case("1024_rows_" + window, s, res, {f: fits["out"][window, f]["g"] for f in ("lean", "plain")}, extra=extra)
    for layer in DENSE:
        print(window, layer, "near-tie gates (row, unit, float64, float32):", ties[layer])
        assert len(forced["other_" + layer]) == 0, (layer, "gates that differ without being near-ties", forced["other_" + layer])
    if (window, form) == ("window0", "lean"):        # the lean form IS plain float32 autograd's gradient on the five tensors
        for name in FIVE:
            scale, kscale, err = apart[name]
            print("window0 %-14s lean - float32 yardstick: %.2e of scale" % (name, err / scale))
            assert err <= 1e-4 * scale + 5e-5 * kscale, (name, "lean against the float32 yardstick", err / scale)
    assert np.isfinite(o["g"]).all() and np.abs(o["g"]).max() > 0
    factor = {name: 2e-3 for name in FIVE} if (window, form) == ("window0", "lean") else None
    check_gradient("%s fp32 yardstick" % window, s, res["float64"]["g"], res["float32"]["g"])
    misses = {}
    for key in ("float64", "float64_fp32gates"):      # a near-tie gate may be decided either way
        ref = res[key]
        misses[key] = check_gradient("%s %s vs %s" % (window, form, key), s, ref["g"], o["g"], factor=factor)
        if not misses[key]:
            check_losses(o["loss"], ref["loss"])
            check_update(s, fits["w"], o["g"], o["w_new"], ref["stats"])
            print(window, form, "meets the bounds against", key)
            return
    assert False, (window, form, misses)
