"""What the tests of the DQN fit share: one seeded gathered minibatch, one fit from a fresh state, the per-tensor bounds
against a float64 gradient and between the lean and the plain form, and the float64 batch statistics of a big
minibatch.  A helper module (not collected): tests and tools/ import from here, never from a test module."""
import numpy as np

from oracle import pyoracle


def collect_minibatch(N, M=4, batch=4, seed=0x0F160077, ticks=10):
    from ofighters_amd import ArenaBatch, DeviceBuffer
    b = ArenaBatch(N, M)
    b.replay_create(16, 0)
    b.spawn_random(seed)
    mask = np.zeros((N, M), np.uint8)
    mask[:, [0, 3]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    for t in range(ticks):
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
    return b, n, rows_d, bp_d, bn_d


def fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs):
    w_d, m_d, v_d, g_d = bufs
    zeros = np.zeros_like(w)
    w_d.upload(w); m_d.upload(zeros); v_d.upload(zeros)
    if kind == "textbook":
        l = b.dqn_fit(w_d, m_d, v_d, 1, 1e-4, n, rows_d.ptr, bp_d.ptr, y.ptr, y2.ptr, g_d)
    else:
        l = b.dqn_fit_reference(w_d, m_d, v_d, 1, 1e-4, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, 0.9, g_d)
    return l, g_d.download(np.float32, w.shape), w_d.download(np.float32, w.shape)


def compare_gradients(shapes, rg, g, loose=()):
    """gradients tensor by tensor: fp32 kernels vs the float64 checker
    (the bias of a convolution that feeds a BatchNorm has an exactly zero gradient: only rounding noise is left, so
    the absolute part of the tolerance is tied to the layer's kernel gradient).
    `loose` layers: a ReLU whose input is within fp32 rounding of zero is gated one way in fp32 and the other way in
    float64; the gradient of that ONE activation then differs by its full value, which shows as a localised error (a few
    cells of u0 and their neighbours through the up-sampling) in the gradients that are short sums.  For those tensors
    the check is on the structure of the error - rms, share of outliers, a cap on the worst element - instead of max."""
    report = []
    for name, (o, shp) in shapes.items():
        c = int(np.prod(shp))
        layer, kind = name.split(".")
        if kind in ("mean", "var"):
            continue
        ref, got = rg[o:o + c], g[o:o + c]
        ko, kshp = shapes[layer + ".kernel"]
        kscale = float(np.abs(rg[ko:ko + int(np.prod(kshp))]).max())
        scale, err = float(np.abs(ref).max()), float(np.abs(got - ref).max())
        if layer in loose:
            tol = 1e-4 * scale + 5e-5 * kscale
            rms = float(np.sqrt(((got - ref) ** 2).mean()))
            outliers = float((np.abs(got - ref) > tol).mean())
            ok = rms <= tol and outliers <= 0.03 and err <= 3e-3 * scale
            report.append((name, scale, err, ok))
            print("%-18s rms %.2e of scale, %.2f %% of the elements above 1e-4, worst %.2e" % (name, rms / scale, 100 * outliers, err / scale))
        else:
            report.append((name, scale, err, err <= 1e-4 * scale + 5e-5 * kscale))
    print("\n".join("%-18s scale %.3e  err %.3e  %s" % r for r in report))
    assert all(r[3] for r in report), [r for r in report if not r[3]]


def check_lean_equals_plain(b, n, rows_d, bp_d, bn_d, loose=frozenset(), loose_both=frozenset()):
    """Both forms of the fit on one minibatch, textbook and reference targets: the per-tensor bounds of
    test_lean_fit_equals_plain_fit, equal moved statistics, and two lean runs give the same bits."""
    from ofighters_amd import DeviceBuffer, _native as nat
    w, shapes = pyoracle.policy_init(5, trained_like=True)
    rs = np.random.RandomState(3)
    y = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    y2 = DeviceBuffer(4 * n).upload(rs.uniform(-1, 2, n).astype(np.float32))
    bufs = tuple(DeviceBuffer(w.nbytes) for _ in range(4))
    for kind in ("textbook", "reference"):
        b.set_option(nat.OPT_FIT_PLAIN, 0)
        la, ga, wa = fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs)
        la2, ga2, wa2 = fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs)
        assert la == la2 and np.array_equal(ga, ga2) and np.array_equal(wa, wa2), "lean fit is not bit-reproducible at %d rows" % n
        b.set_option(nat.OPT_FIT_PLAIN, 1)
        lb, gb, wb = fit_once(b, kind, w, n, rows_d, bp_d, bn_d, y, y2, bufs)
        ga, gb = ga.astype(np.float64), gb.astype(np.float64)
        assert np.isfinite(ga).all() and np.abs(ga).max() > 0
        assert abs(la[0] - lb[0]) <= 1e-5 * max(1.0, abs(lb[0])) and abs(la[1] - lb[1]) <= 1e-5 * abs(lb[1]) + 1e-12, (kind, la, lb)
        bad = []
        for name, (o, shp) in shapes.items():
            c = int(np.prod(shp))
            layer, what = name.split(".")
            if what in ("mean", "var"):
                np.testing.assert_allclose(wa[o:o + c], wb[o:o + c], rtol=1e-5, atol=1e-7, err_msg="%s %s" % (kind, name))
                continue
            ko, kshp = shapes[layer + ".kernel"]
            kscale = float(np.abs(gb[ko:ko + int(np.prod(kshp))]).max())
            scale, err = float(np.abs(gb[o:o + c]).max()), float(np.abs(ga[o:o + c] - gb[o:o + c]).max())
            print("%-10s %-18s scale %.3e  err/scale %.2e" % (kind, name, scale, err / max(scale, 1e-30)))
            if what == "bias" and layer + ".gamma" in shapes:
                # the bias of a convolution in front of a BatchNorm has an EXACTLY zero gradient: what either form delivers
                # is the rounding noise of its sums (it grows with the batch) - bounded against the layer's kernel
                # gradient, not compared element by element
                lean_scale = float(np.abs(ga[o:o + c]).max())
                assert max(scale, lean_scale) <= 2e-4 * kscale, (kind, name, scale, lean_scale, kscale)
                if layer == "conv1":        # the first layer's is written as the exact zero (f_first_bwd_finish)
                    assert lean_scale == 0.0, (kind, name)
            elif err > (2e-3 if ((name in loose and kind == "textbook") or name in loose_both) else 1e-4) * scale + 5e-5 * kscale:
                bad.append((name, scale, err))
        assert not bad, (kind, n, bad)


def batch_statistics_f64(tmp_path, w, shapes, bits, vec8):
    """tests/bn_stats64.py in a process of its own: torch's HIP runtime and libofx's do not initialise side by side in
    one process in that order (torch reports no GPU once libofx has opened the device), and the checker shares nothing
    with the library anyway."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = list(shapes)
    fin, fout = str(tmp_path / "bn_in.npz"), str(tmp_path / "bn_out.npz")
    np.savez(fin, w=w, bits=bits, vec8=vec8, names=np.array(names), offs=np.array([shapes[k][0] for k in names]),
             shp=np.array([list(shapes[k][1]) + [0] * (4 - len(shapes[k][1])) for k in names]))
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "bn_stats64.py"), fin, fout], capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    d = np.load(fout)
    return {k[:-5]: (d[k], d[k[:-5] + ".var"]) for k in d.files if k.endswith(".mean")}
