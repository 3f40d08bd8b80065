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


def sidecar_path(path):
    """The small JSON beside a population checkpoint `path`."""
    return str(path) + ".json"


def population_meta(layers, P, seed):
    return {"layers": [int(v) for v in layers], "P": int(P), "seed": int(seed)}


def check_population_meta(meta, shape, dtype, layers, P, seed, path="the checkpoint"):
    """Population.load's refusals, before a genome is touched: ValueError naming the first field of the sidecar `meta`
    (or of the array: its shape, its dtype) that differs from the population's."""
    want = population_meta(layers, P, seed)
    for field in ("layers", "P", "seed"):
        if field not in meta:
            raise ValueError("%s: the sidecar has no field %r" % (path, field))
        got = [int(v) for v in meta[field]] if field == "layers" else int(meta[field])
        if got != want[field]:
            raise ValueError("%s: %s is %r, this population's is %r" % (path, field, got, want[field]))
    elements = sum(genome_sizes(layers))
    if tuple(shape) != (int(P), elements):
        raise ValueError("%s: shape is %r, a population of P = %d genomes of %d elements is %r"
                         % (path, tuple(shape), P, elements, (int(P), elements)))
    if np.dtype(dtype) != np.float64:
        raise ValueError("%s: dtype is %s, genomes are float64" % (path, np.dtype(dtype)))


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
        self._solution = self._teacher_mask = self._err = self._err_acc = None   # imitate's buffers, made at its first call
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

    def learn(self, solution_ptr, rate, mask_ptr=None, y_ptr=None, err_ptr=None, out_ptr=None):
        """One gradient step per genome toward the device float64 [N][M][4] at solution_ptr (ofx_population_learn): the
        samples of a genome are its live ships whose entry of the device uint8 [N][M] at mask_ptr is set (None: all).
        Writes the actions `act` would have written from the weights before the call (into the batch's action array, or
        out_ptr), so it stands where `act` stood.  err_ptr: device float64 [N][M], the samples' squared errors."""
        self.b.population_learn(self._genome_of.ptr, solution_ptr, rate, mask_ptr=mask_ptr, out_ptr=out_ptr, y_ptr=y_ptr,
                                err_ptr=err_ptr)

    def _imitation_buffers(self):
        from .engine import DeviceBuffer
        if self._solution is None:
            nm = self.b.N * self.b.M
            self._solution, self._teacher_mask = DeviceBuffer(nm * 32), DeviceBuffer(nm)
            self._err = DeviceBuffer(nm * 8).upload(np.full(nm, -1.0))
            self._err_acc = DeviceBuffer(16).upload(np.zeros(2))

    def imitate(self, rate, err_ptr=None):
        """The student flies, the teacher labels: the batch's action array, as bot_actions has just written it for every
        ship, becomes targets and a mask (ofx_population_targets) in buffers the population owns, then `learn` writes
        the evolved ships' own actions in place and moves their genomes toward the teacher's.  err_ptr None: the
        population's own err buffer, reduced on the device into the (sum, count) pair of imitation_error()."""
        self._imitation_buffers()
        self.b.population_targets(self._solution.ptr, self._teacher_mask.ptr)
        self.learn(self._solution.ptr, rate, mask_ptr=self._teacher_mask.ptr, err_ptr=err_ptr or self._err.ptr)
        if err_ptr is None:
            self.b.population_err_reduce(self._err.ptr, self._err_acc.ptr)

    def imitation_error(self, reset=True):
        """(sum of the samples' squared errors, number of samples) of the imitate calls since the last reset.
        Synchronises."""
        self._imitation_buffers()
        self.b.sync()
        acc = self._err_acc.download(np.float64, (2,))
        if reset:
            self._err_acc.upload(np.zeros(2))
        return float(acc[0]), int(acc[1])

    # ------------------------------------------------------------ checkpoint of the whole population
    def save(self, path):
        """Every genome as ONE .npy at `path`, float64 [P][n_weights + n_biases] in the element order, filled slot by slot
        through ofx_population_get into a memory map (a 23 MB genome never exists twice on the host), and the sidecar
        `path + ".json"` with layers, P and seed.  Returns path."""
        import json
        out = np.lib.format.open_memmap(path, mode="w+", dtype=np.float64, shape=(self.P, self.n_weights + self.n_biases))
        for p in range(self.P):
            w, b = self.b.population_get(p, self.n_weights, self.n_biases)
            out[p, :self.n_weights], out[p, self.n_weights:] = w, b
        out.flush()
        del out
        with open(sidecar_path(path), "w") as f:
            json.dump(population_meta(self.layers, self.P, self.seed), f)
        return path

    def load(self, path):
        """The genomes `save` wrote, into this population.  ValueError naming the field, with no genome touched, when the
        checkpoint's layers, P or seed (or the array's shape) differ from this population's."""
        import json
        with open(sidecar_path(path)) as f:
            meta = json.load(f)
        arr = np.load(path, mmap_mode="r")
        check_population_meta(meta, arr.shape, arr.dtype, self.layers, self.P, self.seed, path)
        for p in range(self.P):
            row = np.asarray(arr[p])
            self.b.population_set(p, row[:self.n_weights], row[self.n_weights:])

    def fitness(self, reset=False):
        """After a restart: add what every assigned ship banked to its genome's sum and count."""
        self.b.population_fitness(self._genome_of.ptr, self._sum, self._count, reset)

    def fitness_host(self):
        """(sum int64 [P], count int32 [P]) - the 2 x P numbers a generation brings to the host.  Synchronises."""
        self.b.sync()
        return self._sum.download(np.int64, (self.P,)), self._count.download(np.int32, (self.P,))

    def load_fitness(self, sum, count):
        """Put back what fitness_host returned (a resumed run)."""
        s, c = np.asarray(sum, np.int64), np.asarray(count, np.int32)
        if s.shape != (self.P,) or c.shape != (self.P,):
            raise ValueError("sum and count are [%d] arrays, got %s and %s" % (self.P, s.shape, c.shape))
        self.b.sync()
        self._sum.upload(s)
        self._count.upload(c)

    def imitation_state(self):
        """The running (sum, count) pair of imitation_error as a float64 [2], left as it is.  Synchronises."""
        self._imitation_buffers()
        self.b.sync()
        return self._err_acc.download(np.float64, (2,))

    def load_imitation_state(self, acc):
        a = np.asarray(acc, np.float64)
        if a.shape != (2,):
            raise ValueError("the imitation pair is a float64 [2], got %s" % (a.shape,))
        self._imitation_buffers()
        self.b.sync()
        self._err_acc.upload(a)

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

    Opt-in (a memetic warm start): with imitate_rate > 0, while generation < imitate_generations the hook is
    population.imitate(imitate_rate) instead of population.act - every evolved ship flies on its genome and the genome
    takes one gradient step toward what the ship's own entry of `behaviours` would have done (ofx_population_learn);
    the children are bred from what the parents learned.  The samples' squared errors are reduced on the device and
    `imitation_log` gets (generation, sum, samples) per episode.  The defaults make exactly the calls of before.

    population  a Population on `engine` (or anything with its P, assign, act, fitness, fitness_host and breed; under
                imitation also imitate and imitation_error, for state_dict also load_fitness and the imitation state)
    """

    def __init__(self, engine, population, behaviours, seed, ships=(0,), survivors=1, dafts=0, evolution_rate=0.05,
                 mutation_rate=0.05, episodes_per_generation=1, imitate_rate=0.0, imitate_generations=0, **kw):
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
        self.imitate_rate, self.imitate_generations = float(imitate_rate), int(imitate_generations)
        if not np.isfinite(self.imitate_rate) or self.imitate_rate < 0 or self.imitate_generations < 0:
            raise ValueError("imitate_rate must be finite and >= 0 and imitate_generations >= 0, got %r and %r"
                             % (imitate_rate, imitate_generations))
        self.imitation_log = []           # (generation, summed squared error, samples) per episode that imitated
        self._imitated = False            # the current episode has made an imitate call
        # without imitation the hook is population.act itself: exactly the calls of a run that never heard of it
        self.policy = self._fly if self.imitate_rate > 0 and self.imitate_generations > 0 else population.act
        self._assign()

    def _fly(self, engine):
        """The policy hook under imitation: while generation < imitate_generations the evolved ships fly AND learn, the
        teacher of each being its own entry of `behaviours`, whose action bot_actions has just written."""
        if self.generation < self.imitate_generations:
            self.population.imitate(self.imitate_rate)
            self._imitated = True
        else:
            self.population.act(engine)

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
        if self._imitated:
            err, n = self.population.imitation_error()
            self.imitation_log.append((self.generation, err, n))
            self._imitated = False
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

    # ------------------------------------------------------------ stop and go on
    def state_dict(self):
        """What a run stopped between two lock-steps needs, beside the genomes (Population.save), to go on bit for bit in
        fresh handles: the generation and episode counters, the logs, the plans, the fitness sums and counts of the
        running generation, the imitation pair of the running episode, the tick and ArenaBatch.state_dict()."""
        s, c = self.population.fitness_host()
        d = {"generation": self.generation, "episodes": self.episodes, "tick": self.tick,
             "fitness_log": list(self.fitness_log), "plans": [np.array(p) for p in self.plans],
             "imitation_log": list(self.imitation_log), "score_log": [np.array(t) for t in self.score_log],
             "fitness_sum": s, "fitness_count": c, "imitated": bool(self._imitated), "engine": self.e.state_dict()}
        if self._imitated:
            d["imitation_pair"] = self.population.imitation_state()
        return d

    def load_state_dict(self, d):
        """Continue the run state_dict() described, on a freshly constructed EvolutionRollout with the same arguments
        whose population already holds the genomes (Population.load)."""
        missing = [k for k in ("generation", "episodes", "tick", "fitness_log", "plans", "imitation_log", "score_log",
                               "fitness_sum", "fitness_count", "imitated", "engine") if k not in d]
        if missing:
            raise ValueError("EvolutionRollout.load_state_dict: field %r is missing" % missing[0])
        self.e.load_state_dict(d["engine"])
        self.population.load_fitness(d["fitness_sum"], d["fitness_count"])
        self._imitated = bool(d["imitated"])
        if self._imitated:
            self.population.load_imitation_state(d["imitation_pair"])
        self.generation, self.episodes, self.tick = int(d["generation"]), int(d["episodes"]), int(d["tick"])
        self.fitness_log, self.imitation_log = list(d["fitness_log"]), list(d["imitation_log"])
        self.plans = [np.array(p) for p in d["plans"]]
        self.score_log = [np.array(t) for t in d["score_log"]]
        self._assign()
