"""Seeded evolution strategies on the host, in numpy float64: the reference of tests/test_es.py and tests/test_gpu_es.py.
A helper module (not collected).

Restated from the contract in include/ofx.h ("evolution strategies"; Salimans et al. 2017 with mirrored sampling), not
from the product's code.  A genome is ONE float64 vector in the element order of tests/evolution_oracle.py.

    noise    r0..r3 = Philox4x32-10 of counter (pair i, element e, generation, 12) keyed by the seed;
             S = r0 + r1 + r2 + r3 as an integer;  eps(i, e) = (S - (2^33 - 2)) * 2^-32, exact in float64
    member   m = 2 i + b < P:  w[e] = theta[e] + (s * sigma) * eps(i, e),  s = +1 (b = 0) or -1 (b = 1), the product
             rounded, then the sum;  m = P: the centre itself
    update   g = 0.0;  for i ascending:  g = g + d[i] * eps(i, e);  theta[e] = theta[e] + scale * g
Scalars are drawn through oracle.pyoracle.philox, arrays through tests/boltzmann_oracle.philox_words (held to
pyoracle.philox word for word in tests/test_boltzmann.py).
"""
import numpy as np

from oracle import pyoracle
from tests.boltzmann_oracle import philox_words
from tests.evolution_oracle import decode, forward, fresh, n_elements

STREAM_ES = 12
CENTRE_OF_S = (1 << 33) - 2        # the middle of S's range [0, 2^34 - 4]


def eps_of_words(r):
    """eps of Philox words r [..., 4]: integer arithmetic first, one exact conversion, one exact scaling."""
    S = np.asarray(r, np.uint32).astype(np.int64).sum(axis=-1)
    return (S - CENTRE_OF_S).astype(np.float64) * 2.0 ** -32


def eps(seed, pair, elements, generation):
    """eps(pair, e) for every e of `elements` (an int array) at `generation`."""
    return eps_of_words(philox_words(seed, pair, np.asarray(elements, np.int64), generation, STREAM_ES))


def eps_scalar(seed, pair, e, generation):
    r = pyoracle.philox(int(pair), int(e), int(generation), STREAM_ES, seed)
    return (sum(int(v) for v in r) - CENTRE_OF_S) / 4294967296.0


def _elements(theta, elements):
    return np.arange(theta.size, dtype=np.int64) if elements is None else np.asarray(elements, np.int64)


def member(theta, seed, m, P, sigma, generation, elements=None):
    """Member m of P around `theta` (the centre's values AT `elements` when those are given): an element vector."""
    theta = np.asarray(theta, np.float64)
    assert P >= 2 and P % 2 == 0 and 0 <= m <= P
    if m == P:
        return theta.copy()
    s = np.float64(sigma if m % 2 == 0 else -sigma)
    t = np.multiply(s, eps(seed, m // 2, _elements(theta, elements), generation))      # rounded
    return theta + t                                                                   # rounded


def update(theta, d, scale, seed, generation, elements=None):
    """theta after ofx_es_update (the centre's values AT `elements` when those are given)."""
    theta = np.asarray(theta, np.float64)
    e = _elements(theta, elements)
    g = np.zeros(theta.shape, np.float64)
    for i, di in enumerate(np.asarray(d, np.float64)):
        t = np.multiply(di, eps(seed, i, e, generation))
        g = g + t
    step = np.multiply(np.float64(scale), g)
    return theta + step


def pair_weights(sum, count):
    """(d float64 [P/2], n_c): centred average ranks of the members of complete pairs, written out member by member."""
    n_pairs = len(sum) // 2                                 # a trailing slot P (the centre) is ignored
    complete = [i for i in range(n_pairs) if count[2 * i] > 0 and count[2 * i + 1] > 0]
    members = [2 * i + b for i in complete for b in (0, 1)]
    n_c = len(members)
    d = np.zeros(n_pairs, np.float64)
    if n_c < 2:
        return d, n_c
    mean = {m: int(sum[m]) / int(count[m]) for m in members}
    if len(set(mean.values())) == 1:
        return d, n_c
    u = {}
    for m in members:
        lower = len([q for q in members if mean[q] < mean[m]])
        tied = len([q for q in members if mean[q] == mean[m]])
        rank = lower + (tied - 1) / 2.0                     # the average of ranks lower .. lower + tied - 1
        u[m] = rank / (n_c - 1) - 0.5
    for i in complete:
        d[i] = u[2 * i] - u[2 * i + 1]
    return d, n_c


class OracleES:
    """ofighters_amd.es.ES's interface on the host: the centre held by the oracle, members made when they fly."""

    def __init__(self, batch, layers, seed):
        self.b, self.layers, self.seed = batch, list(layers), int(seed)
        self.theta = fresh(self.layers, seed, 0, 0)
        assert self.theta.size == n_elements(self.layers)
        self.P, self.member_of = None, None
        self.sum = self.count = None
        self.calls = []                 # ("assign", member_of, P) / ("act", tick, sigma, generation) / ("fitness", reset)
        self._members = {}              # / ("update", generation, d, scale)

    def assign(self, member_of, P):
        from ofighters_amd.es import check_member_assignment
        self.member_of = check_member_assignment(member_of, self.b.N, self.b.M, P)
        if P != self.P:
            self.P, self.sum, self.count = P, np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int32)
        self.calls.append(("assign", self.member_of.copy(), P))

    def _member(self, m, sigma, generation):
        key = (m, sigma, generation)
        if key not in self._members:
            self._members[key] = member(self.theta, self.seed, m, self.P, sigma, generation)
        return self._members[key]

    def act(self, sigma, generation):
        b = self.b
        self.calls.append(("act", b.lockstep_count, sigma, generation))
        for a, arena in enumerate(b.arenas):
            alive = arena.ships()["alive"]
            sm, lm = arena.rasterise()
            head, _ = arena.obs_head()
            for i in range(b.M):
                m = self.member_of[a, i]
                if m >= 0 and alive[i]:
                    y = forward(self.layers, self._member(int(m), sigma, generation), head[i], sm, lm)
                    b._acts[a][i] = decode(y, arena.cfg.width, arena.cfg.height)

    def fitness(self, reset=False):
        self.calls.append(("fitness", bool(reset)))
        if reset:
            self.sum[:], self.count[:] = 0, 0
        for a, arena in enumerate(self.b.arenas):
            last = arena.ships()["last_score"]
            for i in range(self.b.M):
                m = self.member_of[a, i]
                if m >= 0:
                    self.sum[m] += last[i]
                    self.count[m] += 1

    def fitness_host(self):
        return self.sum.copy(), self.count.copy()

    def load_fitness(self, sum, count):
        self.sum, self.count = np.array(sum, np.int64), np.array(count, np.int32)

    def update(self, d, lr, sigma, n_c, generation):
        scale = lr / (n_c * sigma)
        self.calls.append(("update", int(generation), np.array(d), scale))
        self.theta = update(self.theta, d, scale, self.seed, generation)
        self._members = {}
