"""tests/fit_ref64.py - the chunked float64 checker of one fit step - checked on the CPU against the small references the
suite already trusts: tests/fit_torch_ref.py::fit_reference (F.conv2d, F.batch_norm in float64) and its options.
Random maps with 3 % of the bits set, weights synthetic(5).

The bound is 1e-10 of the layer's kernel-gradient scale on every tensor: two float64 evaluations of one graph in
different summation orders (measured: worst 7.8e-12 unchunked, 7e-15 chunked against unchunked).

The module takes about half a minute of wall time, not seconds: the graph is fixed at 400 x 400 maps, so a case cannot
be made smaller than its rows, and the two comparisons that set the time are the sizes they are for a reason - 4 rows
is the size of the GPU suite's float64 tests, and 8 rows in chunks of 3 is the smallest split with two full chunks and a
short last one.  Everything else runs on 1 or 2 rows."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle
from tests import fit_ref64 as F64
from tests.fit_torch_ref import fit_reference

BOUND = 1e-10


def _inputs(n, seed):
    from ofighters_amd.agents.policy_weights import synthetic
    _, shapes = pyoracle.policy_init(1)
    w = synthetic(5).astype(np.float64)
    rs = np.random.RandomState(seed)
    x0 = rs.uniform(size=(n, 2, 400, 400)) < 0.03
    bits = np.packbits(x0.reshape(n, 2, 160000), axis=-1, bitorder="little").view(np.uint32).reshape(n, 2, 5000)
    a = dict(bits=bits, vec8=rs.uniform(-1, 1, (n, 8)).astype(np.float32), iaction=rs.randint(0, 2, n).astype(np.int64),
             px=rs.randint(0, 400, n).astype(np.int64), py=rs.randint(0, 400, n).astype(np.int64),
             y_act=rs.uniform(-1, 2, n).astype(np.float32), y_ptr=rs.uniform(-1, 2, n).astype(np.float32))
    return w, shapes, x0.astype(np.float64), a


def _ref(*args, **kw):
    """fit_reference -> (l1, l2, g, stats, e1, e2)"""
    r = fit_reference(*args, **kw)
    return (r["l1"], r["l2"], r["g"], r["stats"]) + ((None, None) if r["e"] is None else (r["e"][:, 0], r["e"][:, 1]))


def _agree(tag, shapes, got, ref_l, ref_g, ref_stats=None):
    """losses, every tensor's gradient and (when given) the batch statistics within BOUND; prints the worst figure"""
    worst = 0.0
    for a, b in zip((got["l1"], got["l2"]), ref_l):
        assert abs(a - b) <= BOUND * max(abs(b), 1e-30), (tag, a, b)
    for name, (o, shp) in shapes.items():
        layer, kind = name.split(".")
        if kind in ("mean", "var"):
            continue
        c = int(np.prod(shp))
        ko, kshp = shapes[layer + ".kernel"]
        kscale = float(np.abs(ref_g[ko:ko + int(np.prod(kshp))]).max())
        assert kscale > 0, (tag, layer)
        err = float(np.abs(got["g"][o:o + c] - ref_g[o:o + c]).max()) / kscale
        worst = max(worst, err)
        assert err <= BOUND, (tag, name, err)
    if ref_stats is not None:
        assert set(ref_stats) == set(got["stats"]) and len(ref_stats) == 7
        for layer, (m, v) in ref_stats.items():
            gm, gv = got["stats"][layer]
            m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
            assert np.abs(gm - m).max() <= BOUND * max(np.abs(m).max(), 1e-30), (tag, layer, "mean")
            assert np.abs(gv - v).max() <= BOUND * max(np.abs(v).max(), 1e-30), (tag, layer, "var")
    print("%s: worst gradient error %.2e of the layer's kernel-gradient scale" % (tag, worst))
    return worst


def test_unchunked_checker_equals_torch_reference_at_4_rows():
    w, shapes, x0, a = _inputs(4, 1)
    l1, l2, g, stats = _ref(w, shapes, x0, a["vec8"], a["iaction"], a["px"], a["py"], a["y_act"], a["y_ptr"])[:4]
    got = F64.fit_step(w, shapes, **a)
    _agree("checker vs fit_reference, 4 rows", shapes, got, (l1, l2), g, stats)
    assert got["e"].shape == (4, 2)
    assert abs((got["e"][:, 0] ** 2).sum() / 8 - l1) <= 1e-12 * l1 and abs((got["e"][:, 1] ** 2).sum() / 640000 - l2) <= 1e-12 * l2


def test_chunked_equals_unchunked():
    """chunks of 3 of 8 rows (3 + 3 + 2: an uneven last chunk): gradient, losses, errors and batch statistics"""
    w, shapes, x0, a = _inputs(8, 2)
    whole = F64.fit_step(w, shapes, **a)
    parts = F64.fit_step(w, shapes, chunk=3, **a)
    _agree("chunked (3 of 8 rows) vs unchunked", shapes, parts, (whole["l1"], whole["l2"]), whole["g"], whole["stats"])
    assert np.abs(parts["e"] - whole["e"]).max() <= BOUND * np.abs(whole["e"]).max()


def test_options_against_the_small_references():
    """legacy bilinear, dense targets, row weights and Huber(delta), each at 2 rows against the reference the suite
    already uses for it (the chunked form: chunk 1)"""
    w, shapes, x0, a = _inputs(2, 3)
    rs = np.random.RandomState(4)
    pos = (a["vec8"], a["iaction"], a["px"], a["py"], a["y_act"], a["y_ptr"])
    l1, l2, g, stats = _ref(w, shapes, x0, *pos, legacy=True)[:4]
    _agree("legacy", shapes, F64.fit_step(w, shapes, legacy=True, chunk=1, **a), (l1, l2), g, stats)
    dense = (rs.uniform(-1, 2, (2, 2)), rs.uniform(-1, 2, (2, 400, 400)))
    l1, l2, g, stats = _ref(w, shapes, x0, a["vec8"], dense=dense)[:4]
    got = F64.fit_step(w, shapes, a["bits"], a["vec8"], dense=dense, chunk=1)
    _agree("dense", shapes, got, (l1, l2), g, stats)
    assert "e" not in got
    row_w = rs.uniform(0.05, 1.0, 2)
    l1, l2, g, _, e1, e2 = _ref(w, shapes, x0, *pos, row_w=row_w)
    got = F64.fit_step(w, shapes, row_w=row_w, chunk=1, **a)
    _agree("row weights", shapes, got, (l1, l2), g)
    assert np.abs(got["e"] - np.stack([e1, e2], 1)).max() <= BOUND * np.abs(e1).max()
    delta = float(np.median(np.abs(np.stack([e1, e2]))))          # errors on both sides of delta
    assert (np.abs(np.stack([e1, e2])) > delta).any() and (np.abs(np.stack([e1, e2])) < delta).any()
    l1, l2, g, _, h1, h2 = _ref(w, shapes, x0, *pos, row_w=row_w, huber_delta=delta)
    got = F64.fit_step(w, shapes, row_w=row_w, huber_delta=delta, chunk=1, **a)
    _agree("row weights + huber", shapes, got, (l1, l2), g)
    assert np.abs(got["e"] - np.stack([h1, h2], 1)).max() <= BOUND * np.abs(h1).max()


def test_diagnostic_forms_force_what_they_say():
    """round_stats and dense_gates (fit_step's docstring), and near_tie_gates' criterion.  The forcing is checked on an
    EXACT tie: with dense2's bias raised by minus the pre-activation of one unit of one row, that gate sits at 0 - relu and
    the mask `> 0` close it, the forced mask opens it, the forward values are the same and the gradients are not."""
    w, shapes, x0, a = _inputs(2, 8)
    base = F64.fit_step(w, shapes, chunk=1, **a)
    own = {k: v > 0 for k, v in base["pre"].items()}
    same = F64.fit_step(w, shapes, chunk=1, dense_gates=own, **a)
    _agree("own gates forced", shapes, same, (base["l1"], base["l2"]), base["g"], base["stats"])
    z = base["pre"]["dense2"]
    row, unit = np.unravel_index(np.abs(z).argmin(), z.shape)
    o, shp = shapes["dense2.bias"]
    assert shp == (50,) and np.abs(base["pre"]["dense2"][1 - row, unit]) > 0
    # one unit's bias moves every row's pre-activation of that unit; only `row` lands on the tie
    w2 = w.copy()
    w2[o + unit] -= z[row, unit]
    tie = F64.fit_step(w2, shapes, chunk=1, **a)
    assert abs(tie["pre"]["dense2"][row, unit]) < 1e-15
    gates = {k: v > 0 for k, v in tie["pre"].items()}
    gates["dense2"][row, unit] = True
    forced = F64.fit_step(w2, shapes, chunk=1, dense_gates=gates, **a)
    assert abs(forced["l1"] - tie["l1"]) <= 1e-12 * abs(tie["l1"])                 # the forward does not move ...
    ko, kshp = shapes["dense2.kernel"]
    diff = np.abs(forced["g"][ko:ko + 5000] - tie["g"][ko:ko + 5000]).max()
    assert diff > 1e-6 * np.abs(tie["g"][ko:ko + 5000]).max(), diff                # ... the gradient does
    # near_tie_gates: a gate that differs counts only when its margin is below twice the layer's largest deviation
    p64 = {"dense2": np.array([[1e-7, 0.5, -2e-7], [0.3, -0.2, 1.0]])}
    p32 = {"dense2": np.array([[-1e-7, -0.5, -1e-7], [0.3 + 3e-7, -0.2, 1.0]])}   # largest deviation: 1.0 at [0][1]
    g, found = F64.near_tie_gates(p64, {"dense2": p32["dense2"]})
    assert found["dense2"][0].shape == (2, 4) and found["dense2"][1].shape == (0, 4)    # both differing gates lie below 2 x 1.0
    p32["dense2"][0, 1] = 0.5                                                          # largest deviation now 3e-7
    g, found = F64.near_tie_gates(p64, p32)
    assert [list(r[:2]) for r in found["dense2"][0]] == [[0, 0]] and not g["dense2"][0, 0] and g["dense2"][0, 1]
    # rounding the batch statistics to float32 moves the gradient a little and not much
    rounded = F64.fit_step(w, shapes, chunk=1, round_stats=True, **a)
    o, shp = shapes["conv2.kernel"]
    err = np.abs(rounded["g"][o:o + 576] - base["g"][o:o + 576]).max() / np.abs(base["g"][o:o + 576]).max()
    print("statistics rounded to float32: conv2.kernel moves by %.2e of scale" % err)
    assert 0 < err < 1e-5
    coef = F64.fit_step(w, shapes, chunk=1, round_stats=True, round_coef=True, **a)
    err2 = np.abs(coef["g"][o:o + 576] - rounded["g"][o:o + 576]).max() / np.abs(base["g"][o:o + 576]).max()
    print("BatchNorm-backward sums rounded to float32 as well: conv2.kernel moves by another %.2e of scale" % err2)
    assert 0 < err2 < 1e-5
    with pytest.raises(ValueError):
        F64.fit_step(w, shapes, a["bits"], a["vec8"], dense=(np.zeros((2, 2)), np.zeros((2, 400, 400))), row_w=np.ones(2))


def test_replay_dense_targets_follow_the_reference_quirks():
    """dense_targets(): Trainer.replay's targets as test_dqn_fit_reference_quirks builds them from policy_ref64.forward"""
    from tests import policy_ref64 as R
    w, shapes, x0, a = _inputs(2, 5)
    _, _, xn, nxt = _inputs(2, 6)
    w32 = pyoracle.policy_init(5, trained_like=True)[0]     # moving statistics that are not (0, 1)
    reward, done, gamma = np.array([0.5, -1.0], np.float32), np.array([0, 1], np.uint8), 0.9
    t1, t2 = F64.dense_targets(w32, shapes, (a["bits"], a["vec8"]), (nxt["bits"], nxt["vec8"]), a["iaction"], a["px"], a["py"],
                               reward, done, gamma, chunk=1)
    for s in range(2):
        a_prev, h_prev = R.forward(x0[s, 0], x0[s, 1], a["vec8"][s][None], w32)
        a_next, h_next = R.forward(xn[s, 0], xn[s, 1], nxt["vec8"][s][None], w32)
        w1, w2 = a_prev[0].copy(), h_prev[0].copy()
        live = 0.0 if done[s] else 1.0
        w1[int(a["iaction"][s] != 0)] = reward[s] + gamma * a_next[0].max() * live
        w2[a["px"][s], a["py"][s]] = reward[s] + gamma * h_next[0].max() * live
        assert np.abs(t1[s] - w1).max() <= 1e-12 * np.abs(w1).max()
        assert np.abs(t2[s] - w2).max() <= 1e-12 * np.abs(w2).max()


def test_file_interface_float32_and_several_cases(tmp_path):
    """python tests/fit_ref64.py in.npz out.npz with two cases in one file, one of them in both dtypes: float32 runs,
    is close to float64 and is not float64; a single-case file (no list) is read too (in this process)."""
    w, shapes, x0, a = _inputs(1, 7)
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fit_ref64.py")
    fin, fout = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    keys = {k: k for k in a}
    F64.save_input(fin, w, shapes, [dict(name="both", dtypes=["float64", "float32"], **keys),
                                    dict(name="legacy", legacy=True, **keys)], **a)
    p = subprocess.run([sys.executable, script, fin, fout], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    res = F64.load_output(fout)
    assert set(res) == {"both", "legacy"} and set(res["both"]) == {"float64", "float32"} and set(res["legacy"]) == {"float64"}
    direct = F64.fit_step(w, shapes, **a)
    r64, r32 = res["both"]["float64"], res["both"]["float32"]
    _agree("file interface", shapes, dict(l1=r64["loss"][0], l2=r64["loss"][1], g=r64["g"], stats=r64["stats"]),
           (direct["l1"], direct["l2"]), direct["g"], direct["stats"])
    assert np.abs(res["legacy"]["float64"]["g"] - r64["g"]).max() > 0
    o, shp = shapes["conv2.kernel"]
    s = slice(o, o + int(np.prod(shp)))
    err = np.abs(r32["g"][s] - r64["g"][s]).max() / np.abs(r64["g"][s]).max()
    print("float32 vs float64 on conv2.kernel: %.2e of scale" % err)
    assert 0 < err <= 1e-3 and r32["loss"][0] != r64["loss"][0]
    assert r64["e"].shape == (1, 2) and float(r64["seconds"]) > 0 and int(r64["peak_bytes"]) >= 0
    F64.save_input(fin, w, shapes, **a)                      # a single-case file, evaluated in this process
    flat = F64.evaluate(np.load(fin), "cpu")
    assert np.array_equal(flat["case.float64.g"], direct["g"]) and flat["case.float64.e"].shape == (1, 2)
