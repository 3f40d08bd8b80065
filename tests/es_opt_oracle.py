"""The optimiser of the ES centre on the host, in numpy float64: the reference of tests/test_es_optimizer.py and
tests/test_gpu_es_optimizer.py.  A helper module (not collected).

Restated from the contract of ofx_es_step in include/ofx.h, not from the product's code.  Per element e, with G_e the
register sum of ofx_es_update (g = 0.0; g = g + d[i] * eps(i, e) over the pairs with d != 0, ascending), every line one
rounded float64 operation:

    ghat = gscale * G_e;  wd = decay * theta;  q = ghat - wd
    t1 = c1 * m;  t2 = k1 * q;  m' = t1 + t2
    momentum:  step = alpha * m';  theta' = theta + step                       (v untouched)
    adam:      qq = q * q;  t3 = c2 * v;  t4 = k2 * qq;  v' = t3 + t4
               r = sqrt(v');  den = r + eps;  quo = m' / den;  step = alpha * quo;  theta' = theta + step

numpy's float64 multiply, add, subtract, divide and sqrt are IEEE 754's correctly rounded operations and numpy never
contracts two of them into one; `step` keeps every intermediate in an array of its own so that no expression holds two
operations.  The noise, `fresh` and the forward come from tests/es_oracle.py and tests/evolution_oracle.py.
"""
import math

import numpy as np

from tests import es_oracle as so

MOMENTUM, ADAM = 1, 2              # OFX_ES_RULE_MOMENTUM, OFX_ES_RULE_ADAM
RULES = {"momentum": MOMENTUM, "adam": ADAM}
# The seed of the GPU loop test (tests/test_gpu_es_optimizer.py, at the LOOP sizes of tests/test_gpu_es.py): chosen so that
# generation 0 of the oracle loop has an untied pair - tests/test_es_optimizer.py holds it to that on the CPU.
LOOP_SEED = 0x0E5090A0


def estimate(shape, d, seed, generation, elements):
    """G_e for every e of `elements`: the pairs with d != 0 in ascending order, from +0.0."""
    g = np.zeros(shape, np.float64)
    for i, di in enumerate(np.asarray(d, np.float64)):
        if di != 0.0:
            t = np.multiply(di, so.eps(seed, i, elements, generation))
            g = g + t
    return g


def step(theta, m, v, d, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, seed, generation, elements=None):
    """(theta', m', v', q, step) after ofx_es_step on the values AT `elements` (all of them when None).  q and step are
    the terms of stats[0] and stats[1]."""
    assert rule in (MOMENTUM, ADAM)
    theta, m, v = (np.asarray(x, np.float64) for x in (theta, m, v))
    e = np.arange(theta.size, dtype=np.int64) if elements is None else np.asarray(elements, np.int64)
    f = np.float64
    g = estimate(theta.shape, d, seed, generation, e)
    ghat = np.multiply(f(gscale), g)
    wd = np.multiply(f(decay), theta)
    q = np.subtract(ghat, wd)
    t1 = np.multiply(f(c1), m)
    t2 = np.multiply(f(k1), q)
    m2 = np.add(t1, t2)
    if rule == MOMENTUM:
        v2 = v.copy()
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
    return np.add(theta, st), m2, v2, q, st


def step_scalar(theta, m, v, G, rule, gscale, decay, alpha, c1, k1, c2, k2, eps):
    """One element in Python floats, one operation per line, from its estimate G: (theta', m', v')."""
    ghat = gscale * G
    wd = decay * theta
    q = ghat - wd
    t1 = c1 * m
    t2 = k1 * q
    m2 = t1 + t2
    if rule == MOMENTUM:
        step = alpha * m2
        return theta + step, m2, v
    qq = q * q
    t3 = c2 * v
    t4 = k2 * qq
    v2 = t3 + t4
    r = math.sqrt(v2)
    den = r + eps
    quo = m2 / den
    step = alpha * quo
    return theta + step, m2, v2


def scalars(optimizer, lr, sigma, n_c, t, beta1, beta2):
    """(gscale, alpha, c1, k1, c2, k2) ES.update passes at step t (1-based), restated from its documentation."""
    gscale = 1.0 / (n_c * sigma)
    k1 = 1.0 - beta1
    k2 = 1.0 - beta2
    alpha = lr if optimizer == "momentum" else lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
    return gscale, alpha, beta1, k1, beta2, k2


def stats(theta2, q, st):
    """(sum q^2, sum step^2, sum theta'^2), each correctly rounded from the float64 terms (math.fsum)."""
    return tuple(math.fsum(np.multiply(x, x).tolist()) for x in (q, st, theta2))


class OptOracleES(so.OracleES):
    """OracleES with ofighters_amd.es.ES's optimiser: update() steps through `step`, with the scalars of `scalars`."""

    def __init__(self, batch, layers, seed, optimizer="adam", beta1=0.9, beta2=0.999, adam_eps=1e-8, weight_decay=0.0):
        super().__init__(batch, layers, seed)
        self.optimizer, self.beta1, self.beta2, self.adam_eps = optimizer, beta1, beta2, adam_eps
        self.weight_decay = weight_decay
        self.m, self.v = np.zeros_like(self.theta), np.zeros_like(self.theta)
        self.opt_steps = 0
        self.last = (0.0, 0.0, 0.0)

    def update(self, d, lr, sigma, n_c, generation):
        self.opt_steps += 1
        sc = scalars(self.optimizer, lr, sigma, n_c, self.opt_steps, self.beta1, self.beta2)
        self.calls.append(("update", int(generation), np.array(d), sc))
        gscale, alpha, c1, k1, c2, k2 = sc
        self.theta, self.m, self.v, q, st = step(self.theta, self.m, self.v, d, RULES[self.optimizer], gscale,
                                                 self.weight_decay, alpha, c1, k1, c2, k2, self.adam_eps, self.seed,
                                                 generation)
        self.last = stats(self.theta, q, st)
        self._members = {}

    def step_stats(self):
        self.calls.append(("step_stats",))
        return self.last
