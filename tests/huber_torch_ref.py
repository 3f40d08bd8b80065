"""float64 torch autograd of the Huber-weighted textbook DQN loss (ofx_dqn_fit_robust): the graph of
tests/per_torch_ref.py restated, with Keras's Huber(delta) in place of the squared error under the project's
normalisation, sum w h(e1) / (2 n) + sum w h(e2) / (160000 n), and the rows' raw errors (e1, e2) of the training-mode
forward."""
import numpy as np


def huber(e, delta):
    """Keras Huber(delta) per element: 0.5 e^2 for |e| <= delta, else delta |e| - 0.5 delta^2 (torch tensors)."""
    import torch
    a = e.abs()
    return torch.where(a <= delta, 0.5 * e * e, delta * a - 0.5 * delta * delta)


def huber_reference(w, shapes, x0, vec8, iaction, px, py, y_act, y_ptr, row_w, delta, legacy=False, backward=True):
    """-> (loss1, loss2, gradient blob, e1, e2); backward=False: the forward only (gradient None) - with zero targets
    e1 / e2 are then the two heads' outputs at the rows' action / pointer."""
    import torch
    import torch.nn.functional as F
    from tests.policy_ref64 import upsample2
    torch.set_num_threads(8)
    dt = torch.float64
    P = {name: torch.tensor(w[o:o + int(np.prod(shp))].reshape(shp), dtype=dt, requires_grad=backward)
         for name, (o, shp) in shapes.items()}
    n = x0.shape[0]

    def block(x, name, up=False):
        if up:
            x = upsample2(x, legacy)
        z = F.conv2d(x, P[name + ".kernel"].permute(3, 2, 0, 1), P[name + ".bias"], padding=1)
        return torch.relu(F.batch_norm(z, None, None, P[name + ".gamma"], P[name + ".beta"], training=True, eps=1e-3))

    x = torch.tensor(x0, dtype=dt)
    for i in (1, 2, 3, 4):
        x = F.max_pool2d(block(x, "conv%d" % i), 2)
    f = torch.cat([torch.tensor(vec8, dtype=dt), x.permute(0, 2, 3, 1).reshape(n, 5000)], dim=1)
    d1 = torch.relu(f @ P["dense1.kernel"] + P["dense1.bias"])
    d2 = torch.relu(d1 @ P["dense2.kernel"] + P["dense2.bias"])
    o1 = d2 @ P["output1.kernel"] + P["output1.bias"]
    u = torch.relu(d1 @ P["updense1.kernel"] + P["updense1.bias"]).reshape(n, 1, 25, 25)
    for j in (1, 2, 3):
        u = block(u, "upconv%d" % j, up=True)
    o2 = F.conv2d(upsample2(u, legacy), P["upconv4.kernel"].permute(3, 2, 0, 1), P["upconv4.bias"], padding=1)
    idx = torch.arange(n)
    e1 = o1[idx, torch.tensor(iaction)] - torch.tensor(np.asarray(y_act, np.float64), dtype=dt)
    e2 = o2[idx, 0, torch.tensor(py), torch.tensor(px)] - torch.tensor(np.asarray(y_ptr, np.float64), dtype=dt)
    rw = torch.tensor(np.asarray(row_w, np.float64), dtype=dt)
    l1, l2 = (rw * huber(e1, delta)).sum() / (2 * n), (rw * huber(e2, delta)).sum() / (160000 * n)
    g = None
    if backward:
        (l1 + l2).backward()
        g = np.zeros_like(w, dtype=np.float64)
        for name, (o, shp) in shapes.items():
            if P[name].grad is not None:
                g[o:o + int(np.prod(shp))] = P[name].grad.detach().cpu().numpy().ravel()
    return float(l1.detach()), float(l2.detach()), g, e1.detach().numpy(), e2.detach().numpy()
