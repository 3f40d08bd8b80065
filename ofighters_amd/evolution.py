"""Device-resident neuroevolution of the scratch MLP: one genome per ship (include/ofx.h, "neuroevolution").

The reference's second learner is its from-scratch network `[Observation.size, 9, 4]` with a genetic algorithm around it:
`Neural_network.generate / evolution / mutate / reproduce / dafts` (agents/neural_network.py:436-478), one network per
ship (lib/battleground.py:52-76) and the four-sigmoid decode of agents/brAIn.py:129-134.  Here the population lives in
HBM, every ship is flown by its own genome in one launch per lock-step, reproduction runs in place on the device and
the only numbers that come back to the host are 2 x P per generation.

    Population        owns the ofx_population_* calls of one ArenaBatch
    truncation_plan   who survives, who is bred from whom, who is replaced by a fresh genome: pure numpy, no randomness
    EvolutionRollout  the generational loop around ShardedRollout's lock-step

Whether the population's fitness rises is an observation (tools/evolution_time.py records it), not a property any test
holds the code to.
"""
import numpy as np

from .rollout import ShardedRollout


def genome_sizes(layers):
    """(number of weights, number of biases) of one genome of the topology `layers`."""
    layers = [int(v) for v in layers]
    return (sum(layers[i] * layers[i + 1] for i in range(len(layers) - 1)), sum(layers[1:]))


def split_genome(layers, weights, biases):
    """The element order -> (weights_layers, biases_layers) in the shapes of the reference's attributes:
    W_l [n_{l+1}][n_l], b_l [n_{l+1}][1] (neural_network.py:108-111)."""
    W, B, wo, bo = [], [], 0, 0
    for i in range(len(layers) - 1):
        nin, nout = int(layers[i]), int(layers[i + 1])
        W.append(np.asarray(weights[wo:wo + nin * nout], np.float64).reshape(nout, nin))
        B.append(np.asarray(biases[bo:bo + nout], np.float64).reshape(nout, 1))
        wo, bo = wo + nin * nout, bo + nout
    return W, B


def join_genome(layers, weights_layers, biases_layers):
    """(weights_layers, biases_layers) -> the element order (flat weights, flat biases); shapes are checked."""
    n = len(layers) - 1
    if len(weights_layers) != n or len(biases_layers) != n:
        raise ValueError("a genome of %d layers has %d weight matrices and %d bias vectors, got %d and %d"
                         % (len(layers), n, n, len(weights_layers), len(biases_layers)))
    W, B = [], []
    for i in range(n):
        w, b = np.asarray(weights_layers[i], np.float64), np.asarray(biases_layers[i], np.float64)
        if w.shape != (layers[i + 1], layers[i]) or b.size != layers[i + 1]:
            raise ValueError("layer %d: weights %s and %d biases, the topology wants (%d, %d) and %d"
                             % (i, w.shape, b.size, layers[i + 1], layers[i], layers[i + 1]))
        W.append(w.ravel())
        B.append(b.ravel())
    return np.concatenate(W), np.concatenate(B)


def check_plan(plan, P):
    """The validity rule of ofx_population_breed, checked before the library sees the plan: int32 [P], every value in
    [-1, P), and the parent of a child keeps its slot (plan[q] == q).  ValueError otherwise; returns the int32 array."""
    a = np.asarray(plan)
    if a.shape != (int(P),) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("a breeding plan is an integer array [%d], got %s %s" % (P, a.dtype, a.shape))
    bad = np.flatnonzero((a < -1) | (a >= P))
    if bad.size:
        raise ValueError("plan[%d] = %d is outside [-1, %d)" % (bad[0], a[bad[0]], P))
    slots = np.arange(P)
    child = np.flatnonzero((a >= 0) & (a != slots))
    orphan = child[a[a[child]] != a[child]]
    if orphan.size:
        p = orphan[0]
        raise ValueError("plan[%d] = %d, but slot %d is not kept (plan[%d] = %d): a parent must keep its slot"
                         % (p, a[p], a[p], a[p], a[a[p]]))
    return np.ascontiguousarray(a, dtype=np.int32)


def check_assignment(genome_of, N, M, P):
    """genome_of as an int32 [N][M] with every value in [-1, P) (-1: the ship is not evolved); ValueError otherwise."""
    a = np.asarray(genome_of)
    if a.shape != (int(N), int(M)) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("genome_of is an integer array [%d][%d], got %s %s" % (N, M, a.dtype, a.shape))
    bad = np.argwhere((a < -1) | (a >= P))
    if bad.size:
        i, j = bad[0]
        raise ValueError("genome_of[%d][%d] = %d is outside [-1, %d)" % (i, j, a[i, j], P))
    return np.ascontiguousarray(a, dtype=np.int32)


def truncation_plan(sum, count, survivors, dafts):
    """Truncation selection as a breeding plan (int32 [P]) from the device's fitness sums.

    1. slots are ranked by mean fitness sum / count, descending; a slot nobody flew (count 0) ranks below every slot that
       was flown; ties go to the lower slot
    2. the best `survivors` keep their slot
    3. the worst `dafts` of the rest become -1 (a fresh genome, the reference's dafts)
    4. every other slot becomes the child of a survivor, dealt round-robin in rank order
    Pure numpy, no randomness.  Every plan it returns passes check_plan."""
    s, c = np.asarray(sum, np.int64), np.asarray(count, np.int64)
    P = s.shape[0]
    if s.shape != (P,) or c.shape != (P,) or P < 1:
        raise ValueError("sum and count are [P] arrays, got %s and %s" % (s.shape, c.shape))
    survivors, dafts = int(survivors), int(dafts)
    if not (1 <= survivors <= P):
        raise ValueError("survivors must be in [1, %d], got %d" % (P, survivors))
    if not (0 <= dafts <= P - survivors):
        raise ValueError("dafts must be in [0, %d], got %d" % (P - survivors, dafts))
    mean = np.where(c > 0, s / np.maximum(c, 1), -np.inf)
    order = np.lexsort((np.arange(P), -mean))           # by -mean, then by slot
    plan = np.empty(P, np.int32)
    keep, rest = order[:survivors], order[survivors:]
    plan[keep] = keep
    bred = rest[:len(rest) - dafts]
    plan[bred] = keep[np.arange(len(bred)) % survivors]
    plan[rest[len(rest) - dafts:]] = -1
    return plan


class Population:
    """P genomes of the scratch MLP `layers` on the device of `batch` (an ArenaBatch), initialised U[-1, 1) from `seed`.

    The draws of init and breed are keyed by (seed, slot, element, generation): a run is reproducible."""

    def __init__(self, batch, layers, P, seed, init=True):
        from .engine import DeviceBuffer
        self.b = batch
        self.layers = [int(v) for v in layers]
        self.P, self.seed = int(P), int(seed)
        self.n_weights, self.n_biases = genome_sizes(self.layers)
        batch.population_create(self.layers, self.P)
        self._genome_of = DeviceBuffer(batch.N * batch.M * 4)
        self._sum = DeviceBuffer(8 * self.P).upload(np.zeros(self.P, np.int64))
        self._count = DeviceBuffer(4 * self.P).upload(np.zeros(self.P, np.int32))
        self.genome_of = None
        self.assign(np.full((batch.N, batch.M), -1, np.int32))
        if init:
            batch.population_init(self.seed, 0)

    def close(self):
        if self.b is not None:
            self.b.population_destroy()
            self.b = None

    # ---------------------------------------------------------------- genomes
    def genome(self, p):
        """(weights_layers, biases_layers) of slot p: lists of numpy arrays in the reference's shapes."""
        if not (0 <= int(p) < self.P):
            raise ValueError("slot %d outside [0, %d)" % (p, self.P))
        return split_genome(self.layers, *self.b.population_get(p, self.n_weights, self.n_biases))

    def set_genome(self, p, weights_layers, biases_layers):
        if not (0 <= int(p) < self.P):
            raise ValueError("slot %d outside [0, %d)" % (p, self.P))
        self.b.population_set(p, *join_genome(self.layers, weights_layers, biases_layers))

    def save_genome(self, p, path):
        """Slot p as a plain .npz: `layers`, W0.., B0.. (the reference's weights_layers / biases_layers)."""
        W, B = self.genome(p)
        d = {"layers": np.asarray(self.layers, np.int64)}
        d.update(("W%d" % i, w) for i, w in enumerate(W))
        d.update(("B%d" % i, b) for i, b in enumerate(B))
        with open(path, "wb") as f:
            np.savez(f, **d)
        return path

    def load_genome(self, p, path):
        with np.load(path) as z:
            if [int(v) for v in z["layers"]] != self.layers:
                raise ValueError("%s holds a genome of layers %s, this population is %s"
                                 % (path, [int(v) for v in z["layers"]], self.layers))
            n = len(self.layers) - 1
            self.set_genome(p, [z["W%d" % i] for i in range(n)], [z["B%d" % i] for i in range(n)])

    # ------------------------------------------------------------ the device calls
    def assign(self, genome_of):
        """Which genome flies which ship: numpy int [N][M], values in [-1, P), checked before the upload."""
        a = check_assignment(genome_of, self.b.N, self.b.M, self.P)
        self.b.sync()
        self._genome_of.upload(a)
        self.genome_of = a

    def act(self, engine=None, y_ptr=None):
        """Overwrite the evolved ships' entries of the batch's action array (after bot_actions, before step)."""
        self.b.population_act(self._genome_of.ptr, y_ptr=y_ptr)

    def fitness(self, reset=False):
        """After a restart: add what every assigned ship banked to its genome's sum and count."""
        self.b.population_fitness(self._genome_of.ptr, self._sum, self._count, reset)

    def fitness_host(self):
        """(sum int64 [P], count int32 [P]) - the 2 x P numbers a generation brings to the host.  Synchronises."""
        self.b.sync()
        return self._sum.download(np.int64, (self.P,)), self._count.download(np.int32, (self.P,))

    def breed(self, plan, evolution_rate, mutation_rate, generation):
        self.b.population_breed(check_plan(plan, self.P), evolution_rate, mutation_rate, self.seed, generation)


class EvolutionRollout(ShardedRollout):
    """The generational loop: every ship of `ships` in every arena is flown by a genome of `population`, the others by
    `behaviours`; at each episode end the restart banks the scores and the fitness call adds them per genome; every
    `episodes_per_generation` episodes the 2 x P fitness numbers come to the host, (best, mean) is appended to
    `fitness_log`, truncation_plan decides and the population breeds in place with generation + 1.

    genome_of[a][ships[k]] = ((arena_base + a) * len(ships) + k + generation) % P: the `+ generation` term rotates the
    assignment, so genomes meet new neighbours.  Runs with observe=False; its policy hook is population.act.  Single
    GPU: with `dist` set it refuses (sum and count are what a multi-GPU form would all-reduce).

    population  a Population on `engine` (or anything with its P, assign, act, fitness, fitness_host and breed)
    """

    def __init__(self, engine, population, behaviours, seed, ships=(0,), survivors=1, dafts=0, evolution_rate=0.05,
                 mutation_rate=0.05, episodes_per_generation=1, **kw):
        if kw.get("dist") is not None:
            raise ValueError("EvolutionRollout runs on one GPU: `dist` must be None")
        if kw.get("policy") is not None or kw.get("observe"):
            raise ValueError("EvolutionRollout sets `policy` and runs with observe=False")
        self.ships = [int(i) for i in ships]
        if not self.ships or len(set(self.ships)) != len(self.ships) or not all(0 <= i < engine.M for i in self.ships):
            raise ValueError("ships must be distinct ship slots in [0, %d), got %r" % (engine.M, list(ships)))
        P = int(population.P)
        truncation_plan(np.zeros(P, np.int64), np.zeros(P, np.int32), survivors, dafts)   # checks both numbers
        if int(episodes_per_generation) < 1:
            raise ValueError("episodes_per_generation must be >= 1, got %r" % (episodes_per_generation,))
        kw["observe"] = False
        super().__init__(engine, behaviours, seed, **kw)
        self.population = population
        self.survivors, self.dafts = int(survivors), int(dafts)
        self.evolution_rate, self.mutation_rate = float(evolution_rate), float(mutation_rate)
        self.episodes_per_generation = int(episodes_per_generation)
        self.generation = 0
        self.episodes = 0                 # finished episodes of the current generation
        self.fitness_log = []             # (best mean fitness of a genome, mean fitness per evolved ship) per generation
        self.plans = []                   # the plan each generation bred on
        self.policy = population.act
        self._assign()

    def assignment(self, generation):
        """genome_of (int32 [N][M]) of `generation` by the formula."""
        e, K = self.e, len(self.ships)
        g = np.full((e.N, e.M), -1, np.int32)
        arena = np.arange(e.arena_base, e.arena_base + e.N, dtype=np.int64)
        for k, ship in enumerate(self.ships):
            g[:, ship] = (arena * K + k + generation) % self.population.P
        return g

    def _assign(self):
        self.population.assign(self.assignment(self.generation))

    def _episode_end(self):
        total = super()._episode_end()
        self.population.fitness(reset=self.episodes == 0)
        self.episodes += 1
        if self.episodes == self.episodes_per_generation:
            s, c = self.population.fitness_host()
            flown = c > 0
            mean = s[flown] / c[flown]
            self.fitness_log.append((float(mean.max()) if flown.any() else float("nan"),
                                     float(s.sum()) / float(max(int(c.sum()), 1))))
            plan = truncation_plan(s, c, self.survivors, self.dafts)
            self.generation += 1
            self.population.breed(plan, self.evolution_rate, self.mutation_rate, self.generation)
            self.plans.append(plan)
            self.episodes = 0
            self._assign()
        return total
