"""torch autograd of ONE fit step of the DQN, the training-mode graph stated once: conv -> BatchNorm on batch statistics
-> ReLU -> pool, the dense layers, the up-sampling head (F.conv2d, F.batch_norm), then the loss on both heads and its
backward.  float64 on the CPU is the checker of ofx_dqn_fit and its weighted / robust / reference forms.  Keras itself
is absent from the image: parity with it is UNPINNED, the conventions are those declared in
ofighters_amd/csrc/ofx_train.hip.  tests/fit_ref64.py states the same graph a second time, independently (nine shifted
matmuls, explicit statistics, chunks); tests/test_fit_ref64.py compares the two."""
import numpy as np


def huber(e, delta):
    """Keras Huber(delta) per element: 0.5 e^2 for |e| <= delta, else delta |e| - 0.5 delta^2 (torch tensors)."""
    import torch
    a = e.abs()
    return torch.where(a <= delta, 0.5 * e * e, delta * a - 0.5 * delta * delta)


def fit_reference(w, shapes, x0, vec8, iaction=None, px=None, py=None, y_act=None, y_ptr=None, *, legacy=False, dense=None,
                  row_w=None, huber_delta=None, dtype=None, backward=True):
    """x0 [n][2][400][400] maps, vec8 [n][8]; the textbook targets are (iaction, px, py, y_act, y_ptr): one error per head
    and row.  dense = (t1 [n][2], t2 [n][400][400]): whole target tensors (ofx_dqn_fit_reference) instead.
    legacy: the TF1 bilinear mapping (OFX_OPT_BILINEAR_LEGACY).  row_w [n]: Keras sample_weight, sum w e1^2 / (2 n) +
    sum w e2^2 / (160000 n) (ofx_dqn_fit_weighted).  huber_delta: Keras Huber(delta) in place of the squared error under
    the same normalisation (ofx_dqn_fit_robust).  dtype: torch.float64 (None: the checker) or torch.float32 (how far
    plain fp32 autograd lands from it).  backward=False: the forward only - with zero targets e is then the two heads'
    outputs at the rows' action / pointer.  An option that is off adds no arithmetic to the graph.
    -> the keys of fit_ref64.fit_step: l1, l2, g (float64 blob, zero where the loss does not reach; None without the
    backward), e [n][2] raw errors of the two heads (None in the dense form), stats {layer: (mean, biased variance)}."""
    import torch
    import torch.nn.functional as F
    from tests.policy_ref64 import upsample2
    if dense is not None and (row_w is not None or huber_delta is not None):
        raise ValueError("fit_reference: row weights and Huber belong to the textbook targets, not to dense ones")
    torch.set_num_threads(8)
    dt = dtype or torch.float64
    P = {name: torch.tensor(w[o:o + int(np.prod(shp))].reshape(shp), dtype=dt, requires_grad=backward)
         for name, (o, shp) in shapes.items()}
    n = x0.shape[0]
    stats = {}

    def out(t):
        return t.detach().double().cpu().numpy()

    def block(x, name, up=False):
        if up:
            x = upsample2(x, legacy)
        z = F.conv2d(x, P[name + ".kernel"].permute(3, 2, 0, 1), P[name + ".bias"], padding=1)           # HWIO -> OIHW
        stats[name] = (out(z.mean(dim=(0, 2, 3))), out(z.var(dim=(0, 2, 3), unbiased=False)))
        return torch.relu(F.batch_norm(z, None, None, P[name + ".gamma"], P[name + ".beta"], training=True, eps=1e-3))

    def tt(a):
        return torch.tensor(np.asarray(a, np.float64), dtype=dt)

    x = torch.tensor(x0, dtype=dt)
    for i in (1, 2, 3, 4):
        x = F.max_pool2d(block(x, "conv%d" % i), 2)
    f = torch.cat([torch.tensor(vec8, dtype=dt), x.permute(0, 2, 3, 1).reshape(n, 5000)], dim=1)   # Flatten order (h, w, c)
    d1 = torch.relu(f @ P["dense1.kernel"] + P["dense1.bias"])
    d2 = torch.relu(d1 @ P["dense2.kernel"] + P["dense2.bias"])
    o1 = d2 @ P["output1.kernel"] + P["output1.bias"]
    u = torch.relu(d1 @ P["updense1.kernel"] + P["updense1.bias"]).reshape(n, 1, 25, 25)
    for j in (1, 2, 3):
        u = block(u, "upconv%d" % j, up=True)
    o2 = F.conv2d(upsample2(u, legacy), P["upconv4.kernel"].permute(3, 2, 0, 1), P["upconv4.bias"], padding=1)
    if dense is not None:
        e1, e2 = o1 - tt(dense[0]), o2[:, 0] - tt(dense[1])
    else:
        idx = torch.arange(n)
        e1 = o1[idx, torch.tensor(iaction)] - tt(y_act)
        e2 = o2[idx, 0, torch.tensor(py), torch.tensor(px)] - tt(y_ptr)

    def terms(e):
        le = e ** 2 if huber_delta is None else huber(e, huber_delta)
        return le if row_w is None else tt(row_w) * le

    l1, l2 = terms(e1).sum() / (2 * n), terms(e2).sum() / (160000 * n)
    g = None
    if backward:
        (l1 + l2).backward()
        g = np.zeros_like(w, dtype=np.float64)
        for name, (o, shp) in shapes.items():
            if P[name].grad is not None:
                g[o:o + int(np.prod(shp))] = out(P[name].grad).ravel()
    return dict(l1=float(l1.detach()), l2=float(l2.detach()), g=g, stats=stats,
                e=np.stack([out(e1), out(e2)], axis=1) if dense is None else None)
