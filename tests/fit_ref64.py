"""float64 checker of ONE fit step of the DQN at any batch size: the training-mode graph of
tests/fit_torch_ref.py::fit_reference (BatchNorm on batch statistics, mse / Huber on both heads) and its backward with
torch autograd, evaluated in chunks of rows so that the peak memory is set by the chunk and not by the minibatch
(the unchunked autograd holds 0.24 GB per row in float64).

How the chunks see the batch statistics.  The seven normalised convolutions lie one behind the other, so layer k's
statistics are a function of the weights and of the statistics of the layers in front of it:
    pass one, per layer k:  (S1, S2) = sum over chunks of (sum (z_k - c), sum (z_k - c)^2), every chunk's term under
                            torch.utils.checkpoint (nothing of the chunk is kept, it is recomputed in the backward);
                            mean = c + S1 / cnt, var = S2 / cnt - (S1 / cnt)^2.  c is a constant close to the mean (the
                            first chunk's own mean, no gradient): the shifted form is exact for any c and keeps the
                            float32 evaluation free of the cancellation of E[z^2] - E[z]^2.
    pass two:               every chunk recomputed with all means and variances as INPUTS -> its share of the loss.
Mean and variance stay nodes of the autograd graph, so the gradient flows through the statistics exactly as in
F.batch_norm(training=True).  The trunk's output (5000 floats per row) and the dense layers are evaluated on the whole
minibatch; the trunk is recomputed five times (four statistics, the output), the up-sampling head four times.

Convolutions are nine shifted matmuls (conv3x3 below, the arithmetic of bn_stats64.conv3x3_f64: MIOpen has no float64
path), the up-sampling is policy_ref64.upsample2.  Stand-alone: imports nothing of libofx.

    python tests/fit_ref64.py in.npz out.npz

in.npz: w, names, offs, shp (the weight blob and its layout, as for bn_stats64.py) and either the arrays of one case under
the names in ARRAYS or `cases`, a JSON list of cases whose array entries name arrays of the file (see evaluate()).
One process evaluates all cases of a file - starting torch on a GPU costs more than the arithmetic.  Runs on `cuda` when
torch sees a device and on the CPU otherwise."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARRAYS = ("bits", "vec8", "iaction", "px", "py", "y_act", "y_ptr", "row_w", "t1", "t2")
EPS = 1e-3
TRUNK = ("conv1", "conv2", "conv3", "conv4")
HEAD = ("upconv1", "upconv2", "upconv3")


def conv3x3(x, k, bias):
    """bn_stats64.conv3x3_f64 - x [n][h][w][ci], k HWIO, zero padding 1, nine shifted matmuls - with every matmul batched
    over (sample, image row).  The forward is the same; the backward's weight gradient is then a batch of n h sums over
    one image row each, added up - not ONE matrix product whose inner dimension is n h w (millions): the BLAS runs that
    in a single workgroup (40 ms per tap on the GPU in float64, 99 % of the checker's time)."""
    import torch.nn.functional as F
    n, h, w_, ci = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    z = bias.reshape(1, 1, 1, -1).expand(n, h, w_, k.shape[3]).clone()
    for ky in range(3):
        for kx in range(3):
            z += xp[:, ky:ky + h, kx:kx + w_, :] @ k[ky, kx].expand(n, h, ci, k.shape[3])
    return z


def fit_step(w, shapes, bits, vec8, iaction=None, px=None, py=None, y_act=None, y_ptr=None, legacy=False, dense=None,
             row_w=None, huber_delta=0.0, dtype="float64", chunk=None, device="cpu", round_stats=False, round_coef=False,
             dense_gates=None):
    """One fit step's losses, gradient, per-row errors and batch statistics.

    bits [n][2][5000] uint32 (bit k of the plane = word k / 32, bit k % 32), vec8 [n][8]; the textbook targets are
    (iaction, px, py, y_act, y_ptr): one error per head and row.  dense = (t1 [n][2], t2 [n][400][400]): whole target
    tensors (ofx_dqn_fit_reference).  row_w [n]: Keras sample_weight; huber_delta > 0: Keras
    Huber(delta) in place of the squared error under the same normalisation (both as in tests/fit_torch_ref.py).
    chunk: rows per chunk (None: the whole minibatch at once, without checkpoints).
    Two diagnostic forms, for telling apart what a float32 evaluation of this graph may do differently:
    round_stats: every BatchNorm's batch mean and variance are rounded to float32 where they are used (the gradient passes
    straight through the rounding) - the forward statistics of an fp32 evaluation inside an otherwise exact one.
    round_coef: the gradients that arrive at every BatchNorm's batch mean and variance - per channel, the two batch-wide
    sums that BatchNorm's backward spreads over all pixels alike - are rounded to float32: its per-channel coefficients
    as an fp32 evaluation would carry them.
    dense_gates {layer: bool [n][units]} for dense1 / dense2 / updense1: the ReLU of that layer is replaced by the given
    0 / 1 mask, fixed in the backward - the decisions of another evaluation forced onto this one.
    -> dict: l1, l2, g (float64 blob, zero where the loss does not reach), e [n][2] (textbook form only), stats
    {layer: (mean, biased variance)}, pre {dense layer: pre-activations [n][units]}."""
    import torch
    from torch.utils.checkpoint import checkpoint
    from tests.policy_ref64 import upsample2
    dev = torch.device(device)
    dt = {"float64": torch.float64, "float32": torch.float32}[dtype]
    n = int(bits.shape[0])
    if dense is not None and (row_w is not None or huber_delta):
        raise ValueError("fit_ref64.fit_step: row weights and Huber belong to the textbook targets, not to dense ones")
    whole = chunk is None or chunk >= n
    step = n if whole else int(chunk)
    spans = [(i, min(i + step, n)) for i in range(0, n, step)]
    P = {name: torch.tensor(np.asarray(w[o:o + int(np.prod(shp))], np.float64).reshape(shp), dtype=dt, device=dev,
                            requires_grad=True) for name, (o, shp) in shapes.items()}

    def run(fn, *args):
        return fn(*args) if whole else checkpoint(fn, *args, use_reentrant=False)

    def unpack(lo, hi):   # [c][2][5000] uint32 words -> [c][400][400][2]
        t = torch.from_numpy(bits[lo:hi].view(np.int32).astype(np.int64) & 0xFFFFFFFF).to(dev)
        sh = torch.arange(32, device=dev, dtype=torch.int64)
        return ((t.unsqueeze(-1) >> sh) & 1).reshape(hi - lo, 2, 400, 400).permute(0, 2, 3, 1).to(dt)

    def conv(x, name):
        return conv3x3(x, P[name + ".kernel"], P[name + ".bias"])

    def bn_relu(z, name, mean, var):
        return torch.relu((z - mean) / torch.sqrt(var + EPS) * P[name + ".gamma"] + P[name + ".beta"])

    def pool(x):
        m, h, w_, c = x.shape
        return x.reshape(m, h // 2, 2, w_ // 2, 2, c).amax(dim=(2, 4))

    def up(x):
        return upsample2(x.permute(0, 3, 1, 2), legacy).permute(0, 2, 3, 1)

    def trunk_z(x, k, st):
        """z of TRUNK[k] from the chunk's maps, given the statistics of the layers in front (st: flat mean, var, ...)"""
        for i in range(k):
            x = pool(bn_relu(conv(x, TRUNK[i]), TRUNK[i], st[2 * i], st[2 * i + 1]))
        return conv(x, TRUNK[k])

    def head_z(u, k, st):
        """z of HEAD[k] (k = 3: the output convolution upconv4) from the chunk's u0"""
        for i in range(k):
            u = bn_relu(conv(up(u), HEAD[i]), HEAD[i], st[2 * i], st[2 * i + 1])
        return conv(up(u), "upconv4" if k == 3 else HEAD[k])

    def statistics(zfn, inputs, st):
        """mean and biased variance of zfn(input, *st) over all chunks, as nodes of the graph"""
        with torch.no_grad():
            z = zfn(inputs[0], *st)
            c, cnt = z.mean(dim=(0, 1, 2)), n * z.shape[1] * z.shape[2]
            del z

        def sums(x, *s):
            d = zfn(x, *s) - c
            return d.sum(dim=(0, 1, 2)), (d * d).sum(dim=(0, 1, 2))

        s1 = s2 = 0
        for x in inputs:
            a, b = run(sums, x, *st)
            s1, s2 = s1 + a, s2 + b
        mean, var = c + s1 / cnt, s2 / cnt - (s1 / cnt) ** 2
        if round_coef:
            mean.register_hook(lambda gr: gr.float().to(dt))
            var.register_hook(lambda gr: gr.float().to(dt))
        if round_stats:
            mean = mean + (mean.float().to(dt) - mean).detach()
            var = var + (var.float().to(dt) - var).detach()
        return mean, var

    pre = {}

    def dense_relu(x, name):
        z = x @ P[name + ".kernel"] + P[name + ".bias"]
        pre[name] = z.detach().double().cpu().numpy()
        if dense_gates is not None and name in dense_gates:
            return z * torch.tensor(np.asarray(dense_gates[name]), dtype=dt, device=dev)
        return torch.relu(z)

    stats = {}
    maps = [unpack(lo, hi) for lo, hi in spans]      # 1-bit maps: no gradient, kept for the five trunk passes
    st = []
    for k, name in enumerate(TRUNK):
        mean, var = statistics(lambda x, *s, k=k: trunk_z(x, k, s), maps, st)
        stats[name] = (mean, var)
        st += [mean, var]
    flat = torch.cat([run(lambda x, *s: pool(bn_relu(trunk_z(x, 3, s), "conv4", s[6], s[7])).reshape(x.shape[0], 5000), x, *st)
                      for x in maps])                  # Flatten order (h, w, c)
    del maps
    f = torch.cat([torch.tensor(np.asarray(vec8, np.float64), dtype=dt, device=dev), flat], dim=1)
    d1 = dense_relu(f, "dense1")
    d2 = dense_relu(d1, "dense2")
    o1 = d2 @ P["output1.kernel"] + P["output1.bias"]
    u0 = dense_relu(d1, "updense1").reshape(n, 25, 25, 1)
    us = [u0[lo:hi] for lo, hi in spans]
    st = []
    for k, name in enumerate(HEAD):
        mean, var = statistics(lambda x, *s, k=k: head_z(x, k, s), us, st)
        stats[name] = (mean, var)
        st += [mean, var]

    def tt(a, kind=None):
        return torch.tensor(np.asarray(a), dtype=kind or dt, device=dev)

    def loss_of(e, lo, hi):
        """the rows' terms of the loss before the heads' normalisation 1 / (2 n) and 1 / (160000 n): e^2, or Keras
        Huber(delta) - 0.5 e^2 inside delta, delta |e| - 0.5 delta^2 beyond - times the rows' weights"""
        if huber_delta:
            a = e.abs()
            le = torch.where(a <= huber_delta, 0.5 * e * e, huber_delta * a - 0.5 * huber_delta * huber_delta)
        else:
            le = e * e
        return le * rw[lo:hi] if rw is not None else le

    rw = tt(row_w) if row_w is not None else None
    idx = torch.arange(n, device=dev)
    if dense is not None:
        e1 = o1 - tt(dense[0])
    else:
        e1 = o1[idx, tt(iaction, torch.int64)] - tt(y_act)
    l1 = loss_of(e1, 0, n).sum() / (2 * n)
    l2, e2s = 0, []
    for (lo, hi), u in zip(spans, us):
        if dense is not None:
            def part(u, *s, lo=lo, hi=hi):
                e = head_z(u, 3, s)[..., 0] - tt(dense[1][lo:hi])
                return (e * e).sum() / (160000 * n), e.detach()
        else:
            def part(u, *s, lo=lo, hi=hi):
                e = head_z(u, 3, s)[torch.arange(hi - lo, device=dev), tt(py[lo:hi], torch.int64), tt(px[lo:hi], torch.int64), 0] \
                    - tt(y_ptr[lo:hi])
                return loss_of(e, lo, hi).sum() / (160000 * n), e.detach()
        l, e = run(part, u, *st)
        l2 = l2 + l
        if dense is None:
            e2s.append(e.detach())
    (l1 + l2).backward()
    g = np.zeros(len(w), np.float64)
    for name, (o, shp) in shapes.items():
        if P[name].grad is not None:
            g[o:o + int(np.prod(shp))] = P[name].grad.detach().double().cpu().numpy().ravel()
    out = dict(l1=float(l1.detach()), l2=float(l2.detach()), g=g, pre=pre,
               stats={k: (m.detach().double().cpu().numpy(), v.detach().double().cpu().numpy()) for k, (m, v) in stats.items()})
    if dense is None:
        out["e"] = np.stack([e1.detach().double().cpu().numpy(), torch.cat(e2s).double().cpu().numpy()], axis=1)
    return out


def dense_targets(w, shapes, rows_prev, rows_next, iaction, px, py, reward, done, gamma, device="cpu", chunk=32):
    """The dense targets of Trainer.replay as written (qlearnIA_V2.py:251-270, tests/test_train.py::
    test_dqn_fit_reference_quirks): the float64 INFERENCE-mode predictions of `state` with target[iaction != 0] and
    ptr_target[px][py] (row x, column y - the quirk) replaced by reward + gamma * max(prediction(next_state)) * (not
    done).  rows_prev / rows_next = (bits, vec8).  -> t1 [n][2], t2 [n][400][400] float64."""
    import torch
    from tests.policy_ref64 import upsample2
    dev, dt = torch.device(device), torch.float64
    P = {name: torch.tensor(np.asarray(w[o:o + int(np.prod(shp))], np.float64).reshape(shp), dtype=dt, device=dev)
         for name, (o, shp) in shapes.items()}

    def block(x, name):
        z = conv3x3(x, P[name + ".kernel"], P[name + ".bias"])
        return torch.relu((z - P[name + ".mean"]) / torch.sqrt(P[name + ".var"] + EPS) * P[name + ".gamma"] + P[name + ".beta"])

    def up(x):
        return upsample2(x.permute(0, 3, 1, 2), False).permute(0, 2, 3, 1)

    def predict(bits, vec8):
        m = bits.shape[0]
        t = torch.from_numpy(bits.view(np.int32).astype(np.int64) & 0xFFFFFFFF).to(dev)
        sh = torch.arange(32, device=dev, dtype=torch.int64)
        x = ((t.unsqueeze(-1) >> sh) & 1).reshape(m, 2, 400, 400).permute(0, 2, 3, 1).to(dt)
        for name in TRUNK:
            x = block(x, name)
            x = x.reshape(m, x.shape[1] // 2, 2, x.shape[2] // 2, 2, 8).amax(dim=(2, 4))
        f = torch.cat([torch.tensor(np.asarray(vec8, np.float64), dtype=dt, device=dev), x.reshape(m, 5000)], dim=1)
        d1 = torch.relu(f @ P["dense1.kernel"] + P["dense1.bias"])
        d2 = torch.relu(d1 @ P["dense2.kernel"] + P["dense2.bias"])
        u = torch.relu(d1 @ P["updense1.kernel"] + P["updense1.bias"]).reshape(m, 25, 25, 1)
        for name in HEAD:
            u = block(up(u), name)
        heat = conv3x3(up(u), P["upconv4.kernel"], P["upconv4.bias"])[..., 0]
        return d2 @ P["output1.kernel"] + P["output1.bias"], heat

    n = rows_prev[0].shape[0]
    t1, t2 = np.zeros((n, 2)), np.zeros((n, 400, 400))
    with torch.no_grad():
        for lo in range(0, n, chunk):
            hi = min(lo + chunk, n)
            a_prev, h_prev = predict(rows_prev[0][lo:hi], rows_prev[1][lo:hi])
            a_next, h_next = predict(rows_next[0][lo:hi], rows_next[1][lo:hi])
            t1[lo:hi], t2[lo:hi] = a_prev.cpu().numpy(), h_prev.cpu().numpy()
            live = 1.0 - np.asarray(done[lo:hi], np.float64)
            r = np.asarray(reward[lo:hi], np.float64)
            s = np.arange(lo, hi)
            t1[s, (np.asarray(iaction[lo:hi]) != 0).astype(np.int64)] = r + gamma * a_next.amax(dim=1).cpu().numpy() * live
            t2[s, np.asarray(px[lo:hi]), np.asarray(py[lo:hi])] = r + gamma * h_next.amax(dim=(1, 2)).cpu().numpy() * live
    return t1, t2


def near_tie_gates(pre64, pre32):
    """The dense ReLU gates of the float64 evaluation with the NEAR-TIES taken the float32 evaluation's way.  A gate counts
    as a near-tie only if the two evaluations decide it differently and its float64 margin |pre-activation| is below twice
    the largest deviation of the float32 pre-activations of that layer from the float64 ones on this batch.
    -> ({layer: bool [n][units]}, {layer: (forced [k][4] = row, unit, float64 value, float32 value; the same for gates that
    differ WITHOUT being near-ties - left as float64 has them)})"""
    gates, found = {}, {}
    for layer, z64 in pre64.items():
        z32 = pre32[layer]
        differ = (z64 > 0) != (z32 > 0)
        near = differ & (np.abs(z64) < 2 * np.abs(z32 - z64).max())
        gates[layer] = np.where(near, z32 > 0, z64 > 0)
        found[layer] = tuple(np.array([[r, u, z64[r, u], z32[r, u]] for r, u in zip(*np.nonzero(m))], np.float64).reshape(-1, 4)
                             for m in (near, differ & ~near))
    return gates, found


def evaluate(d, device):
    """All cases of a loaded input file -> the flat dict written to the output file.

    A case is a dict: name; array entries (ARRAYS) naming arrays of the file; legacy, huber_delta, chunk; dtypes (a list,
    default ["float64"]); variants (a list of "fp32stats", "fp32coef", "fp32gates": float64 evaluations with round_stats, with round_stats
    and round_coef, and with the
    near-tie dense gates of near_tie_gates() taken from the case's float32 evaluation - both dtypes must be listed); replay = {bits_next, vec8_next, reward, done, gamma} (names of arrays, gamma a number): the
    dense targets are then dense_targets() of the case's (bits, vec8) = NEXT state and (bits_prev, vec8_prev)."""
    import torch
    shapes = {str(k): (int(o), tuple(int(v) for v in s if v)) for k, o, s in zip(d["names"], d["offs"], d["shp"])}
    if "cases" in d.files:
        cases = json.loads(str(d["cases"]))
    else:
        cases = [dict(name="case", **{k: k for k in ARRAYS if k in d.files})]
    out = {}
    for c in cases:
        a = {k: d[c[k]] for k in ARRAYS if k in c}
        dense = (a["t1"], a["t2"]) if "t1" in a else None
        if "replay" in c:
            r = c["replay"]
            dense = dense_targets(d["w"], shapes, (d[r["bits_prev"]], d[r["vec8_prev"]]), (a["bits"], a["vec8"]), a["iaction"],
                                  a["px"], a["py"], d[r["reward"]], d[r["done"]], float(r["gamma"]), device=device)
        done = {}

        def one(key, dtype, **more):
            if device == "cuda":
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            t0 = time.time()
            r = fit_step(d["w"], shapes, a["bits"], a["vec8"], a.get("iaction"), a.get("px"), a.get("py"), a.get("y_act"),
                         a.get("y_ptr"), legacy=bool(c.get("legacy", False)), dense=dense, row_w=a.get("row_w"),
                         huber_delta=float(c.get("huber_delta", 0.0)), dtype=dtype, chunk=c.get("chunk"), device=device, **more)
            if device == "cuda":
                torch.cuda.synchronize()
            done[key] = r
            key = "%s.%s." % (c["name"], key)
            out[key + "loss"] = np.array([r["l1"], r["l2"]])
            out[key + "g"] = r["g"]
            if "e" in r:
                out[key + "e"] = r["e"]
            for layer, (m, v) in r["stats"].items():
                out[key + layer + ".mean"], out[key + layer + ".var"] = m, v
            for layer, z in r["pre"].items():
                out[key + "minpre_" + layer] = np.abs(z).min(axis=1)
            out[key + "seconds"] = np.array(time.time() - t0)
            out[key + "peak_bytes"] = np.array(torch.cuda.max_memory_allocated() if device == "cuda" else 0, np.int64)
            return key

        for dtype in c.get("dtypes", ["float64"]):
            one(dtype, dtype)
        for variant in c.get("variants", []):
            if variant == "fp32stats":
                one("float64_fp32stats", "float64", round_stats=True)
            elif variant == "fp32coef":
                one("float64_fp32coef", "float64", round_stats=True, round_coef=True)
            elif variant == "fp32gates":
                gates, found = near_tie_gates(done["float64"]["pre"], done["float32"]["pre"])
                key = one("float64_fp32gates", "float64", dense_gates=gates)
                for layer, rec in found.items():
                    out[key + "forced_" + layer], out[key + "other_" + layer] = rec
            else:
                raise ValueError("fit_ref64: unknown variant %r" % variant)
    return out


def save_input(path, w, shapes, cases=None, **arrays):
    """Write an input file: the weight blob with its layout, the arrays, and the list of cases (None: one case)."""
    names = list(shapes)
    extra = {} if cases is None else {"cases": np.array(json.dumps(cases))}
    np.savez(path, w=np.asarray(w, np.float64), names=np.array(names), offs=np.array([shapes[k][0] for k in names]),
             shp=np.array([list(shapes[k][1]) + [0] * (4 - len(shapes[k][1])) for k in names]), **extra, **arrays)


def load_output(path):
    """{case: {dtype or variant: dict(loss, g, e, seconds, peak_bytes, minpre_<layer>, forced_<layer>, other_<layer>,
    stats {layer: (mean, var)})}}"""
    d = np.load(path)
    res = {}
    for k in d.files:
        case, dtype, what = k.split(".", 2)
        r = res.setdefault(case, {}).setdefault(dtype, {"stats": {}})
        if what.endswith((".mean", ".var")):
            layer, kind = what.split(".")
            pair = r["stats"].setdefault(layer, [None, None])
            pair[kind == "var"] = d[k]
        else:
            r[what] = d[k]
    return res


if __name__ == "__main__":
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    np.savez(sys.argv[2], **evaluate(np.load(sys.argv[1]), "cuda" if torch.cuda.is_available() else "cpu"))
