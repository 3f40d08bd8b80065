"""What the float64 comparisons of the DQN fit at training batch sizes share (tests/test_gpu_fit_fp64.py states the
bounds): the checker's child process, the fit's buffers, the per-tensor checks and the report.  A helper module (not
collected)."""
import json
import os
import subprocess
import sys
import time

import numpy as np

from tests.policy_fp64_cases import REPORT as POLICY_REPORT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(os.path.dirname(POLICY_REPORT), "fit_fp64_report.json")     # the suite's one report folder
LR = 1e-4


def report(tag, rec):
    try:
        os.makedirs(os.path.dirname(REPORT), exist_ok=True)
        data = json.load(open(REPORT)) if os.path.exists(REPORT) else {}
        data[tag] = rec
        json.dump(data, open(REPORT, "w"), indent=1)
    except OSError:
        pass


def run_checker(tmp, w, shapes, cases, arrays, timeout):
    """tests/fit_ref64.py on all cases in a process of its own (one child; a failure or a timeout fails the caller,
    nothing retries) -> fit_ref64.load_output()'s dict, and the child's wall time"""
    from tests import fit_ref64 as F64
    fin, fout = str(tmp / "fit64_in.npz"), str(tmp / "fit64_out.npz")
    F64.save_input(fin, w, shapes, cases, **arrays)
    t0 = time.time()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fit_ref64.py"), fin, fout], capture_output=True, text=True,
                       timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return F64.load_output(fout), time.time() - t0


def fit_buffers(w):
    from ofighters_amd import DeviceBuffer
    return tuple(DeviceBuffer(w.nbytes) for _ in range(4))


def reset_buffers(bufs, w):
    zeros = np.zeros_like(w)
    bufs[0].upload(w); bufs[1].upload(zeros); bufs[2].upload(zeros)


def tensor_errors(shapes, ref_g, g):
    """{tensor: (scale, kscale, err)} of a gradient blob against the float64 one"""
    out = {}
    for name, (o, shp) in shapes.items():
        layer, kind = name.split(".")
        if kind in ("mean", "var"):
            continue
        c = int(np.prod(shp))
        ko, kshp = shapes[layer + ".kernel"]
        kscale = float(np.abs(ref_g[ko:ko + int(np.prod(kshp))]).max())
        out[name] = (float(np.abs(ref_g[o:o + c]).max()), kscale, float(np.abs(g[o:o + c].astype(np.float64) - ref_g[o:o + c]).max()))
    return out


def check_gradient(tag, shapes, ref_g, g, loose_layers=(), factor=None, widened=None):
    """The gradient bounds of the module docstring.  factor {tensor: f}: f * scale in place of 1e-4 * scale for the tensors
    named (only the (1024, 0) allowance of test_lean_fit_equals_plain_fit_large_batches uses it).  widened {tensor: f}:
    err <= f * scale, four times the float32 yardstick's own error, for tensors on which the yardstick itself is beyond half
    the project's bound (the caller asserts that it is).  -> the misses"""
    bad = []
    for name, (scale, kscale, err) in tensor_errors(shapes, ref_g, g).items():
        layer, kind = name.split(".")
        o, shp = shapes[name]
        got, ref = g[o:o + int(np.prod(shp))].astype(np.float64), ref_g[o:o + int(np.prod(shp))]
        if kind == "bias" and layer + ".gamma" in shapes:
            ok = float(np.abs(got).max()) <= 2e-4 * kscale
        elif widened and name in widened:
            ok = err <= widened[name] * scale
        elif layer in loose_layers:
            tol = 1e-4 * scale + 5e-5 * kscale
            rms = float(np.sqrt(((got - ref) ** 2).mean()))
            ok = rms <= tol and float((np.abs(got - ref) > tol).mean()) <= 0.03 and err <= 3e-3 * scale
        else:
            ok = err <= (factor or {}).get(name, 1e-4) * scale + 5e-5 * kscale
        print("%-28s %-18s scale %.3e  err/scale %.2e  err/kscale %.2e %s" % (tag, name, scale, err / max(scale, 1e-30),
                                                                             err / max(kscale, 1e-30), "" if ok else "  <-- MISS"))
        if not ok:
            bad.append((name, scale, kscale, err))
    return bad


def check_losses(l, ref):
    rl1, rl2 = float(ref[0]), float(ref[1])
    assert abs(l[0] - rl1) <= 1e-4 * max(1.0, abs(rl1)) and abs(l[1] - rl2) <= 1e-4 * max(1e-9, abs(rl2)) + 1e-12, (l, rl1, rl2)


def check_update(shapes, w, g, w_new, stats):
    """Adam step 1 from the device's own gradient (test_dqn_fit_vs_torch_autograd) and the moved statistics against the
    float64 batch statistics (test_lean_fit_at_4096_rows)"""
    lr_t = LR * np.sqrt(1 - 0.999) / (1 - 0.9)
    g = g.astype(np.float64)
    for name, (o, shp) in shapes.items():
        c = int(np.prod(shp))
        layer, kind = name.split(".")
        if kind in ("mean", "var"):
            batch_stat = np.asarray(stats[layer][kind == "var"], np.float64)
            want = 0.99 * w[o:o + c].astype(np.float64) + 0.01 * batch_stat
            moved = w_new[o:o + c].astype(np.float64) - 0.99 * w[o:o + c]
            scale = max(float(np.abs(batch_stat).max()), 1e-6)
            err = float(np.abs(moved / 0.01 - batch_stat).max())
            assert err <= 2e-4 * scale + 2e-5, (layer, kind, err, scale)
            np.testing.assert_allclose(w_new[o:o + c], want, rtol=5e-6, atol=1e-6)
        else:
            gi = g[o:o + c]
            want = w[o:o + c] - lr_t * (0.1 * gi) / (np.sqrt(0.001 * gi * gi) + 1e-7)
            np.testing.assert_allclose(w_new[o:o + c], want, rtol=0, atol=2e-7 + 1e-6 * np.abs(w[o:o + c]).max(), err_msg=name)


def report_case(tag, shapes, res, forms, extra=None):
    """per tensor: scale, the forms' errors and the float32 yardstick's, all against float64"""
    ref = res["float64"]["g"]
    cols = {form: tensor_errors(shapes, ref, g) for form, g in forms.items()}
    cols["fp32"] = tensor_errors(shapes, ref, res["float32"]["g"])
    rec = {name: dict(scale=v[0], kscale=v[1], **{form: cols[form][name][2] for form in cols})
           for name, v in cols["fp32"].items()}
    rec["_loss"] = dict(float64=[float(x) for x in res["float64"]["loss"]], fp32=[float(x) for x in res["float32"]["loss"]])
    rec["_checker"] = {dt: dict(seconds=float(res[dt]["seconds"]), peak_gb=float(res[dt]["peak_bytes"]) / 2 ** 30) for dt in res}
    rec.update(extra or {})
    report(tag, rec)
