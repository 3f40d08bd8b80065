"""Per-element adaptive sigma of the ES centre on the host, in numpy float64: the reference of tests/test_es_sigma.py and
tests/test_gpu_es_sigma.py.  A helper module (not collected).

Restated from the contract of ofx_es_sigma_* in include/ofx.h (parameter-exploring policy gradients with symmetric
sampling, Sehnke et al. 2010), not from the product's code, on top of tests/es_oracle.py (the noise) and
tests/es_opt_oracle.py (the optimiser's scalars).  Per element e, every line one rounded float64 operation:

    member   w[e] = theta[e] + (s * sigma[e]) * eps(i, e),  s = +1 or -1; member P is the centre
    step     g = 0.0; qs = 0.0; for the pairs with d != 0 or s != 0, ascending:
                 x = eps(j, e);  t = d[j] * x;  g = g + t;  xx = x * x;  c = xx - THIRD;  u = s[j] * c;  qs = qs + u
             sg = sigma * g;  ghat = gscale * sg;  wd = decay * theta;  q = ghat - wd
             PLAIN: step = alpha * q;  MOMENTUM / ADAM: tests/es_opt_oracle.py's lines from t1 on
             theta' = theta + step
             r = srate * qs;  f = 1.0 + r;  sn = sigma * f;  clamp to [smin, smax];  sigma' = sn

numpy never contracts two operations into one; every intermediate below lives in an array of its own.
"""
import math

import numpy as np

from tests import es_opt_oracle as oo
from tests import es_oracle as so

PLAIN, MOMENTUM, ADAM = 0, oo.MOMENTUM, oo.ADAM
RULES = {None: PLAIN, "momentum": MOMENTUM, "adam": ADAM}
THIRD = float.fromhex("0x1.5555555555555p-2")
# The seed of the GPU loop test (tests/test_gpu_es_sigma.py, at the LOOP sizes of tests/test_gpu_es.py): the optimiser
# loop's, whose generation 0 has an untied pair (tests/test_es_optimizer.py holds it to that).
LOOP_SEED = oo.LOOP_SEED


def _elements(theta, elements):
    return np.arange(theta.size, dtype=np.int64) if elements is None else np.asarray(elements, np.int64)


def member(theta, sigma, seed, m, P, generation, elements=None):
    """Member m of P around `theta` under the vector `sigma` (both AT `elements` when those are given)."""
    theta, sigma = np.asarray(theta, np.float64), np.asarray(sigma, np.float64)
    assert P >= 2 and P % 2 == 0 and 0 <= m <= P and sigma.shape == theta.shape
    if m == P:
        return theta.copy()
    ss = np.multiply(np.float64(1.0 if m % 2 == 0 else -1.0), sigma)                   # exact: a sign
    t = np.multiply(ss, so.eps(seed, m // 2, _elements(theta, elements), generation))  # rounded
    return np.add(theta, t)                                                            # rounded


def sums(shape, d, s, seed, generation, elements):
    """(g, qs) for every e of `elements`: the pairs with d != 0 or s != 0 in ascending order, both from +0.0."""
    g, qs = np.zeros(shape, np.float64), np.zeros(shape, np.float64)
    for i, (di, si) in enumerate(zip(np.asarray(d, np.float64), np.asarray(s, np.float64))):
        if di != 0.0 or si != 0.0:
            x = so.eps(seed, i, elements, generation)
            t = np.multiply(di, x)
            g = np.add(g, t)
            xx = np.multiply(x, x)
            c = np.subtract(xx, np.float64(THIRD))
            u = np.multiply(si, c)
            qs = np.add(qs, u)
    return g, qs


def step(theta, sigma, m, v, d, s, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax, seed, generation,
         elements=None):
    """(theta', sigma', m', v', q, step, clamped) after ofx_es_sigma_step on the values AT `elements` (all when None).
    q, step and clamped (1.0 where a clamp changed the element) are the terms of stats[0], [1] and [4]."""
    assert rule in (PLAIN, MOMENTUM, ADAM)
    theta, sigma, m, v = (np.asarray(x, np.float64) for x in (theta, sigma, m, v))
    f = np.float64
    g, qs = sums(theta.shape, d, s, seed, generation, _elements(theta, elements))
    sg = np.multiply(sigma, g)
    ghat = np.multiply(f(gscale), sg)
    wd = np.multiply(f(decay), theta)
    q = np.subtract(ghat, wd)
    m2, v2 = m.copy(), v.copy()
    if rule == PLAIN:
        st = np.multiply(f(alpha), q)
    else:
        t1 = np.multiply(f(c1), m)
        t2 = np.multiply(f(k1), q)
        m2 = np.add(t1, t2)
        if rule == MOMENTUM:
            st = np.multiply(f(alpha), m2)
        else:
            qq = np.multiply(q, q)
            t3 = np.multiply(f(c2), v)
            t4 = np.multiply(f(k2), qq)
            v2 = np.add(t3, t4)
            r = np.sqrt(v2)
            den = np.add(r, f(eps))
            quo = np.divide(m2, den)
            st = np.multiply(f(alpha), quo)
    theta2 = np.add(theta, st)
    r = np.multiply(f(srate), qs)
    fac = np.add(f(1.0), r)
    sn = np.multiply(sigma, fac)
    low = sn < smin
    sn = np.where(low, f(smin), sn)
    high = sn > smax
    sn = np.where(high, f(smax), sn)
    return theta2, sn, m2, v2, q, st, (low | high).astype(np.float64)


def storage_order(layers):
    """perm with stored[p] = element_vector[perm[p]]: the first layer input-major (position k * n1 + o holds element
    o * nin + k), everything behind it in the element order."""
    nin, n1 = int(layers[0]), int(layers[1])
    n_w = sum(int(a) * int(b) for a, b in zip(layers[:-1], layers[1:]))
    G = n_w + sum(int(b) for b in layers[1:])
    perm = np.arange(G, dtype=np.int64)
    perm[:nin * n1] = np.arange(nin * n1, dtype=np.int64).reshape(n1, nin).T.ravel()
    return perm


def fixed_order_sum(terms, layers):
    """The sum of the element vector `terms` in the library's order: 256 consecutive STORAGE positions per workgroup
    (past G: +0.0) added as a pairwise tree, stride 128, 64, .. 1; then thread t of one workgroup adds the workgroup
    sums t, t + 256, ... from 0.0 and the 256 thread sums are added in thread order."""
    x = np.asarray(terms, np.float64)[storage_order(layers)]
    nb = (x.size + 255) // 256
    x = np.concatenate([x, np.zeros(nb * 256 - x.size)]).reshape(nb, 256)
    stride = 128
    while stride:
        x = np.add(x[:, :stride], x[:, stride:2 * stride])
        stride >>= 1
    part = x[:, 0]
    rounds = (nb + 255) // 256
    part = np.concatenate([part, np.zeros(rounds * 256 - nb)]).reshape(rounds, 256)    # a thread past nb adds nothing:
    a = np.zeros(256, np.float64)                                                       # a + (+0.0) keeps a's bits
    for row in part:
        a = np.add(a, row)
    t = float(a[0])
    for q in range(1, 256):
        t = t + float(a[q])
    return t


def stats(theta2, sigma2, q, st, clamped, layers):
    """The five statistics of a full-genome step in the library's fixed order."""
    return (fixed_order_sum(np.multiply(q, q), layers), fixed_order_sum(np.multiply(st, st), layers),
            fixed_order_sum(np.multiply(theta2, theta2), layers), fixed_order_sum(np.multiply(sigma2, sigma2), layers),
            fixed_order_sum(clamped, layers))


def pair_utilities(sum, count):
    """(d, s, n_c): centred average ranks of the members of complete pairs, member by member; d_i = u_2i - u_2i+1 and
    s_i = u_2i + u_2i+1 (the baseline of centred ranks is 0)."""
    n_pairs = len(sum) // 2                                 # a trailing slot P (the centre) is ignored
    complete = [i for i in range(n_pairs) if count[2 * i] > 0 and count[2 * i + 1] > 0]
    members = [2 * i + b for i in complete for b in (0, 1)]
    n_c = len(members)
    d, s = np.zeros(n_pairs, np.float64), np.zeros(n_pairs, np.float64)
    if n_c < 2:
        return d, s, n_c
    mean = {m: int(sum[m]) / int(count[m]) for m in members}
    if len(set(mean.values())) == 1:
        return d, s, n_c
    u = {}
    for m in members:
        lower = len([q for q in members if mean[q] < mean[m]])
        tied = len([q for q in members if mean[q] == mean[m]])
        rank = lower + (tied - 1) / 2.0
        u[m] = rank / (n_c - 1) - 0.5
    for i in complete:
        d[i] = u[2 * i] - u[2 * i + 1]
        s[i] = u[2 * i] + u[2 * i + 1]
    return d, s, n_c


def scalars(optimizer, lr, n_c, t, beta1, beta2, sigma_lr):
    """(gscale, alpha, c1, k1, c2, k2, srate) ES.update passes in adaptive mode at step t, restated from its
    documentation: sigma[e] is inside the law, so gscale = 1 / n_c; PLAIN steps by lr itself."""
    if optimizer is None:
        return 1.0 / n_c, lr, 0.0, 1.0, 0.0, 1.0, sigma_lr / n_c
    _, alpha, c1, k1, c2, k2 = oo.scalars(optimizer, lr, 1.0, n_c, t, beta1, beta2)
    return 1.0 / n_c, alpha, c1, k1, c2, k2, sigma_lr / n_c


class SigmaOracleES(so.OracleES):
    """OracleES with ofighters_amd.es.ES's adaptive interface: sigma is None at every call, update() takes s."""
    adaptive = True

    def __init__(self, batch, layers, seed, sigma_init, sigma_lr=0.2, sigma_min=None, sigma_max=None, optimizer=None,
                 beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0):
        super().__init__(batch, layers, seed)
        self.sigma_vec = np.full(self.theta.shape, float(sigma_init))
        self.sigma_lr = sigma_lr
        self.sigma_min = sigma_init / 64 if sigma_min is None else sigma_min
        self.sigma_max = sigma_init * 4 if sigma_max is None else sigma_max
        self.optimizer, self.beta1, self.beta2, self.adam_eps = optimizer, beta1, beta2, adam_eps
        self.weight_decay = weight_decay
        self.m, self.v = np.zeros_like(self.theta), np.zeros_like(self.theta)
        self.opt_steps = 0
        self.last = (0.0,) * 5

    def _member(self, m, sigma, generation):
        assert sigma is None, "an adaptive ES flies with its own sigma"
        key = (m, generation)
        if key not in self._members:
            self._members[key] = member(self.theta, self.sigma_vec, self.seed, m, self.P, generation)
        return self._members[key]

    def update(self, d, lr, sigma, n_c, generation, s=None):
        assert sigma is None and s is not None
        if self.optimizer is not None:
            self.opt_steps += 1
        sc = scalars(self.optimizer, lr, n_c, self.opt_steps, self.beta1, self.beta2, self.sigma_lr)
        self.calls.append(("update", int(generation), np.array(d), np.array(s), sc))
        gscale, alpha, c1, k1, c2, k2, srate = sc
        out = step(self.theta, self.sigma_vec, self.m, self.v, d, s, RULES[self.optimizer], gscale, self.weight_decay,
                   alpha, c1, k1, c2, k2, self.adam_eps, srate, self.sigma_min, self.sigma_max, self.seed, generation)
        self.theta, self.sigma_vec, self.m, self.v, q, st, clamped = out
        self.last = stats(self.theta, self.sigma_vec, q, st, clamped, self.layers)
        self._members = {}

    def step_stats(self):
        self.calls.append(("step_stats",))
        return self.last
