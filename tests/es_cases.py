"""What tests/test_gpu_es.py, tests/test_gpu_es_optimizer.py and tests/test_gpu_es_sigma.py share: the seed and the small
arena of their one-ship cases, the bit comparison, and an ES's vectors as element vectors.  A helper module (not
collected), beside tests/evolution_cases.py."""
import ctypes as C

import numpy as np

SEED = 0x0E5090FF
W, H = 48, 40
NIN = 8 + 2 * W * H
HIDDEN = [(9,), (13, 7)]


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def make(hidden, optimizer=None, N=1, M=1, **kw):
    """(batch, ES, layers): an ES of the hidden widths `hidden` on an N x M batch of the small arena."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    layers = [NIN] + list(hidden) + [4]
    b = ArenaBatch(N, M, width=W, height=H)
    return b, ES(b, layers, SEED, optimizer=optimizer, **kw), layers


def state(es):
    """(theta, m, v) of an ES as element vectors, through ofx_es_get and ofx_es_opt_get - (theta, sigma, m, v), sigma
    through ofx_es_sigma_get, when the ES adapts sigma.  m and v are None without optimiser state."""
    b, nw, nb = es.b, es.n_weights, es.n_biases
    m = v = None
    if es.optimizer is not None:
        m, v = (np.concatenate(x) for x in b.es_opt_get(nw, nb))
    theta = np.concatenate(b.es_get(nw, nb))
    if not es.adaptive:
        return theta, m, v
    return theta, np.concatenate(b.es_sigma_get(nw, nb)), m, v


def set_state(es, theta, *rest):
    """Put back what state() returned: set_state(es, *state(es)); trailing m, v may be left out or None."""
    nw = es.n_weights
    es.b.es_set(theta[:nw], theta[nw:])
    if es.adaptive:
        sigma, rest = rest[0], rest[1:]
        es.b.es_sigma_set(sigma[:nw], sigma[nw:])
    m, v = rest if rest else (None, None)
    if m is not None:
        es.b.es_opt_set(m[:nw], m[nw:], v[:nw], v[nw:])


def same(got, want, what):
    """Two state() tuples are equal on every bit; a vector neither has (None in both) is passed over."""
    names = ("theta", "sigma", "m", "v") if len(got) == 4 else ("theta", "m", "v")
    for g, w, name in zip(got, want, names):
        if g is None and w is None:
            continue
        diff = int((bits(g) != bits(w)).sum())
        assert diff == 0, "%s: %s differs in %d of %d elements (max |diff| %.3e)" % (what, name, diff, g.size,
                                                                                    float(np.max(np.abs(g - w))))
