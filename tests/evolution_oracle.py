"""Neuroevolution of the scratch MLP on the host, in numpy float64: the reference of tests/test_evolution.py and
tests/test_gpu_evolution.py.  A helper module (not collected).

Restated from the contract in include/ofx.h ("neuroevolution"), which cites the reference: Neural_network.__init__'s
U[-1, 1) (agents/neural_network.py:108-111), evolution / mutate / reproduce / dafts (:436-478), feed (:396-420) and the
four-sigmoid decode of agents/brAIn.py:129-134.

A genome is ONE float64 vector in the element order: every W_l row-major [n_{l+1}][n_l], layer by layer, then every
bias.  Element e of slot p at `generation` draws from Philox4x32-10 keyed by the seed with counter (p, e, generation,
stream): stream 9 the evolution coefficient (words 0, 1) and the mutation selector (words 2, 3), stream 10 the
replacement value, stream 11 a fresh genome.  Scalars are drawn through oracle.pyoracle.philox, arrays through
tests/boltzmann_oracle.philox_words (held to pyoracle.philox word for word in tests/test_boltzmann.py).
"""
import numpy as np

from oracle import pyoracle
from tests.boltzmann_oracle import philox_words
from tests.oracle_batch import OracleBatch

STREAM_EVOLVE, STREAM_MUTATE, STREAM_FRESH = 9, 10, 11


def u(r_hi, r_lo):
    """numpy's 53-bit uniform double in [0, 1) from two 32-bit words; exact in float64."""
    hi = (np.asarray(r_hi, np.uint64) >> np.uint64(5)).astype(np.float64)
    lo = (np.asarray(r_lo, np.uint64) >> np.uint64(6)).astype(np.float64)
    return (hi * 67108864.0 + lo) / 9007199254740992.0


def n_elements(layers):
    return sum(layers[i] * layers[i + 1] + layers[i + 1] for i in range(len(layers) - 1))


def fresh(layers, seed, p, generation, elements=None):
    """A fresh genome of slot p: 2 u - 1 on stream 11 (init at generation 0, plan[p] == -1 at the breed's generation)."""
    e = np.arange(n_elements(layers), dtype=np.int64) if elements is None else np.asarray(elements, np.int64)
    r = philox_words(seed, p, e, generation, STREAM_FRESH)
    return 2.0 * u(r[..., 0], r[..., 1]) - 1.0


def fresh_scalar(seed, p, e, generation):
    r = pyoracle.philox(p, e, generation, STREAM_FRESH, seed)
    return 2.0 * float(u(r[0], r[1])) - 1.0


def selector(layers, seed, p, generation):
    """u_sel of every element of slot p: an element mutates iff u_sel < mutation_rate."""
    r = philox_words(seed, p, np.arange(n_elements(layers), dtype=np.int64), generation, STREAM_EVOLVE)
    return u(r[..., 2], r[..., 3])


def child(parent, seed, p, generation, evolution_rate, mutation_rate):
    """deepcopy(parent).evolution(rate).mutate(rate) for slot p, element by element."""
    w = np.array(parent, dtype=np.float64)
    e = np.arange(w.size, dtype=np.int64)
    r = philox_words(seed, p, e, generation, STREAM_EVOLVE)
    if evolution_rate > 0:
        c = (2.0 * u(r[..., 0], r[..., 1]) - 1.0) * evolution_rate
        w = np.multiply(c, w) + w                      # three separately rounded operations
    if mutation_rate > 0:
        sel = u(r[..., 2], r[..., 3]) < mutation_rate
        s = philox_words(seed, p, e[sel], generation, STREAM_MUTATE)
        w[sel] = 2.0 * u(s[..., 0], s[..., 1]) - 1.0
    return w


def check_plan(plan, P):
    plan = np.asarray(plan)
    assert plan.shape == (P,) and ((plan >= -1) & (plan < P)).all()
    for p, q in enumerate(plan):
        assert q == -1 or q == p or plan[q] == q, "the parent of slot %d is not kept" % p


def breed(genomes, plan, evolution_rate, mutation_rate, seed, generation, layers):
    """The population after ofx_population_breed: a list of element vectors."""
    check_plan(plan, len(genomes))
    out = []
    for p, q in enumerate(plan):
        if q == p:
            out.append(genomes[p])
        elif q == -1:
            out.append(fresh(layers, seed, p, generation))
        else:
            out.append(child(genomes[q], seed, p, generation, evolution_rate, mutation_rate))
    return out


def split(layers, g):
    """Element vector -> (weights_layers, biases_layers) in the reference's shapes."""
    W, B, o = [], [], 0
    for i in range(len(layers) - 1):
        n = layers[i] * layers[i + 1]
        W.append(g[o:o + n].reshape(layers[i + 1], layers[i]))
        o += n
    for i in range(len(layers) - 1):
        B.append(g[o:o + layers[i + 1]].reshape(layers[i + 1], 1))
        o += layers[i + 1]
    assert o == g.size
    return W, B


def forward(layers, g, head8, ship_map, laser_map):
    """Neural_network.feed on toVector's [head | ship_map.ravel() | laser_map.ravel()]: a <- sigmoid(W a + b) per layer.
    The first layer's binary tail is summed over its set columns (numpy's pairwise sum)."""
    W, B = split(layers, g)
    tail = np.concatenate([np.asarray(ship_map).ravel(), np.asarray(laser_map).ravel()]) != 0
    z = W[0][:, :8] @ np.asarray(head8, np.float64) + W[0][:, 8:][:, tail].sum(axis=1)
    a = 1.0 / (1.0 + np.exp(-(z + B[0][:, 0])))
    for w, b in zip(W[1:], B[1:]):
        a = 1.0 / (1.0 + np.exp(-(w @ a + b[:, 0])))
    return a


def decode(y, W, H):
    """brAIn.py:129-134 with the arena's size in place of 400: (valid, shoot, thrust, px, py); no clamp."""
    return np.array([1, y[0] > 0.5, y[1] > 0.5, int(y[2] * W), int(y[3] * H)], np.int32)


class OraclePopulation:
    """ofighters_amd.evolution.Population's interface on the host: the population held by the oracle."""

    def __init__(self, batch, layers, P, seed):
        self.b, self.layers, self.P, self.seed = batch, list(layers), int(P), int(seed)
        self.genomes = [fresh(self.layers, seed, p, 0) for p in range(self.P)]
        self.genome_of = None
        self.sum, self.count = np.zeros(self.P, np.int64), np.zeros(self.P, np.int32)
        self.calls = []                                 # ("act", tick) / ("fitness", reset) / ("breed", generation)

    def assign(self, genome_of):
        from ofighters_amd.evolution import check_assignment
        self.genome_of = check_assignment(genome_of, self.b.N, self.b.M, self.P)
        self.calls.append(("assign", self.genome_of.copy()))

    def act(self, engine=None):
        b = self.b
        self.calls.append(("act", b.lockstep_count))
        for a, arena in enumerate(b.arenas):
            alive = arena.ships()["alive"]
            sm, lm = arena.rasterise()
            head, _ = arena.obs_head()
            for i in range(b.M):
                g = self.genome_of[a, i]
                if g >= 0 and alive[i]:
                    y = forward(self.layers, self.genomes[g], head[i], sm, lm)
                    b._acts[a][i] = decode(y, arena.cfg.width, arena.cfg.height)

    def fitness(self, reset=False):
        self.calls.append(("fitness", bool(reset)))
        if reset:
            self.sum[:], self.count[:] = 0, 0
        for a, arena in enumerate(self.b.arenas):
            last = arena.ships()["last_score"]
            for i in range(self.b.M):
                g = self.genome_of[a, i]
                if g >= 0:
                    self.sum[g] += last[i]
                    self.count[g] += 1

    def fitness_host(self):
        return self.sum.copy(), self.count.copy()

    def breed(self, plan, evolution_rate, mutation_rate, generation):
        from ofighters_amd.evolution import check_plan as product_check
        plan = product_check(plan, self.P)
        self.calls.append(("breed", int(generation), plan.copy()))
        self.genomes = breed(self.genomes, plan, evolution_rate, mutation_rate, self.seed, generation, self.layers)


class EvolutionOracleBatch(OracleBatch):
    """OracleBatch on small arenas, with the global arena id EvolutionRollout keys the assignment by."""

    def __init__(self, n_arenas, n_ships, width, height, arena_base=0):
        super().__init__(n_arenas, n_ships, arena_base)
        self.arenas = [pyoracle.Arena(cfg=pyoracle.default_cfg(n_ships, width=width, height=height))
                       for _ in range(n_arenas)]
        self.arena_base, self.W, self.H = arena_base, width, height
        self.lockstep_count = 0

    def step(self):
        super().step()
        self.lockstep_count += 1
