"""The learning step of the scratch MLP on the host, in numpy float64: the reference of tests/test_population_learn.py
and tests/test_gpu_population_learn.py.  A helper module (not collected).

Written from the contract of ofx_population_learn / ofx_population_targets in include/ofx.h, which cites the
reference's Neural_network.backprop (agents/neural_network.py:338-393), update_network (:241-300) and
update_network_continuous (:319-334).  A genome is the element vector of tests/evolution_oracle.py; an observation is
(head8, ship_map, laser_map), toVector's [head | ship_map.ravel() | laser_map.ravel()] with a binary tail.
"""
import numpy as np

from tests import evolution_oracle as eo


def obs_vector(head8, ship_map, laser_map):
    """toVector as one dense float64 vector."""
    return np.concatenate([np.asarray(head8, np.float64), np.asarray(ship_map, np.float64).ravel() != 0,
                           np.asarray(laser_map, np.float64).ravel() != 0]).astype(np.float64)


def activations(layers, g, x):
    """[a_0 = x, a_1, ..., a_L] of the dense observation vector x.  The first layer's binary tail is summed over its set
    columns as evolution_oracle.forward does (the same numbers: a_L is that function's result)."""
    W, B = eo.split(layers, g)
    tail = x[8:] != 0
    z = W[0][:, :8] @ x[:8] + W[0][:, 8:][:, tail].sum(axis=1)
    acts = [x, 1.0 / (1.0 + np.exp(-(z + B[0][:, 0])))]
    for w, b in zip(W[1:], B[1:]):
        acts.append(1.0 / (1.0 + np.exp(-(w @ acts[-1] + b[:, 0]))))
    return acts


def deltas(layers, g, acts, solution):
    """(d = solution - a_L, [delta_1 .. delta_L]): delta_L = d * (a_L (1 - a_L)), delta_l = (W_{l+1}^T delta_{l+1}) *
    (a_l (1 - a_l)) with the sum over o ascending, every product and sum rounded on its own."""
    W, _ = eo.split(layers, g)
    a = acts[-1]
    d = np.asarray(solution, np.float64) - a
    out = [d * (a * (1.0 - a))]
    for l in range(len(W) - 1, 0, -1):
        nxt = out[0]
        s = W[l][0, :] * nxt[0]
        for o in range(1, W[l].shape[0]):
            s = s + W[l][o, :] * nxt[o]
        a = acts[l]
        out.insert(0, s * (a * (1.0 - a)))
    return d, out


def err_of(d):
    return ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]


def gradient(layers, g, x, solution):
    """Neural_network.backprop's (gradient_weights, gradient_biases) in its sign: the DESCENT direction's opposite is
    what update_network adds, so these are delta_l a_{l-1}^T and delta_l, the negative gradient of 1/2 sum d^2."""
    acts = activations(layers, g, x)
    _, dl = deltas(layers, g, acts, solution)
    return [np.outer(dl[l], acts[l]) for l in range(len(dl))], [v.reshape(-1, 1) for v in dl]


def learn(layers, g, samples, rate, travel=None):
    """One ofx_population_learn step of one genome.  samples: [(x dense vector, solution [4])] in ascending ship order.
    Every delta comes from the OLD weights; then, sample after sample, w <- w + (c * delta[o]) * a[k], b <- b + c *
    delta[o], c = rate / n.  In the first layer only the head columns and the set columns are touched.
    travel: an element vector of zeros that receives, per element, the sum of the magnitudes of the terms added to it.
    Returns (new element vector, err per sample, a_L per sample)."""
    g = np.asarray(g, np.float64)
    n = len(samples)
    new = g.copy()
    errs, ys = [], []
    TW, TB = eo.split(layers, np.zeros_like(g) if travel is None else travel)
    if n == 0:
        return new, errs, ys
    c = rate / float(n)
    terms = []
    for x, sol in samples:
        acts = activations(layers, g, x)
        d, dl = deltas(layers, g, acts, sol)
        errs.append(err_of(d))
        ys.append(acts[-1])
        terms.append((acts, dl))
    if rate == 0:
        return new, errs, ys
    W, B = eo.split(layers, new)              # views of `new`
    for acts, dl in terms:
        for l in range(len(W)):
            cd = c * dl[l]
            if l == 0:
                x = acts[0]
                W[0][:, :8] += np.outer(cd, x[:8])
                TW[0][:, :8] += np.abs(np.outer(cd, x[:8]))
                cols = 8 + np.flatnonzero(x[8:] != 0)
                W[0][:, cols] += cd[:, None]
                TW[0][:, cols] += np.abs(cd)[:, None]
            else:
                W[l] += np.outer(cd, acts[l])
                TW[l] += np.abs(np.outer(cd, acts[l]))
            B[l][:, 0] += cd
            TB[l][:, 0] += np.abs(cd)
    return new, errs, ys


def targets(action, W, H):
    """ofx_population_targets of one (valid, shoot, thrust, px, py): (solution [4], mask)."""
    valid, shoot, thrust, px, py = [int(v) for v in action]
    cl = lambda v: min(max(v, 0.0), 1.0)
    return (np.array([1.0 if shoot else 0.0, 1.0 if thrust else 0.0, cl((px + 0.5) / float(W)), cl((py + 0.5) / float(H))]),
            valid != 0)


def learn_population(layers, genomes, genome_of, alive, obs, solution, mask, rate, travel=None):
    """The whole call on the host.  travel: None or a list of zero element vectors, one per genome (see learn).  genomes: list of element vectors; genome_of [N][M]; alive [N][M]; obs[a] =
    (head [M][8], ship_map, laser_map); solution [N][M][4]; mask [N][M] or None.
    Returns (new genomes, err {(a, i): value} of the samples, y {(a, i): a_L} of the samples)."""
    N, M = genome_of.shape
    P = len(genomes)
    per = {p: [] for p in range(P)}
    for a in range(N):
        for i in range(M):
            p = int(genome_of[a, i])
            if 0 <= p < P and alive[a, i] and (mask is None or mask[a, i]):
                head, sm, lm = obs[a]
                per[p].append(((a, i), obs_vector(head[i], sm, lm), np.asarray(solution[a, i], np.float64)))
    out, err, y = [], {}, {}
    for p in range(P):
        new, errs, ys = learn(layers, genomes[p], [(x, s) for _, x, s in per[p]], rate,
                              None if travel is None else travel[p])
        out.append(new)
        for (key, _, _), e, v in zip(per[p], errs, ys):
            err[key], y[key] = e, v
    return out, err, y


class LearnOraclePopulation(eo.OraclePopulation):
    """OraclePopulation with Population.learn / imitate / imitation_error on the host."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.err_sum, self.err_count = 0.0, 0

    def _obs(self):
        out, alive = [], []
        for arena in self.b.arenas:
            sm, lm = arena.rasterise()
            head, _ = arena.obs_head()
            out.append((head, sm, lm))
            alive.append(arena.ships()["alive"])
        return out, np.array(alive)

    def learn(self, solution, rate, mask=None):
        """As Population.learn, with host arrays; the evolved ships' actions are written as `act` writes them."""
        b = self.b
        obs, alive = self._obs()
        eo.OraclePopulation.act(self)
        self.calls.pop()                                      # (that was the forward of this call, not an act call)
        self.genomes, err, _ = learn_population(self.layers, self.genomes, self.genome_of, alive, obs, solution, mask, rate)
        return err

    def imitate(self, rate):
        b = self.b
        self.calls.append(("imitate", b.lockstep_count))
        sol, mask = np.zeros((b.N, b.M, 4)), np.zeros((b.N, b.M), bool)
        for a, arena in enumerate(b.arenas):
            for i in range(b.M):
                sol[a, i], mask[a, i] = targets(b._acts[a][i], arena.cfg.width, arena.cfg.height)
        err = self.learn(sol, rate, mask)
        for key in sorted(err):
            self.err_sum += err[key]
        self.err_count += len(err)
        return err

    def imitation_error(self, reset=True):
        out = (self.err_sum, self.err_count)
        if reset:
            self.err_sum, self.err_count = 0.0, 0
        return out

    def imitation_state(self):
        return np.array([self.err_sum, float(self.err_count)])

    def load_imitation_state(self, acc):
        self.err_sum, self.err_count = float(acc[0]), int(acc[1])

    def load_fitness(self, sum, count):
        self.sum[:], self.count[:] = sum, count


# ---------------------------------------------------------------- the exactly rounded twin and the tolerances
def learn_exact(layers, g, samples, rate):
    """`learn` with every dot product of the forward and of the backward pass summed by math.fsum (products rounded
    once, the bias inside the sum) and math.exp: the high-precision twin.  The apply is the contract's, term by term."""
    import math
    g = np.asarray(g, np.float64)
    n = len(samples)
    new = g.copy()
    if n == 0 or rate == 0:
        return new
    c = rate / float(n)
    W, B = eo.split(layers, g)
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    terms = []
    for x, sol in samples:
        cells = 8 + np.flatnonzero(x[8:] != 0)
        a = [sig(math.fsum([float(W[0][o, k]) * float(x[k]) for k in range(8)] + W[0][o, cells].tolist()
                           + [float(B[0][o, 0])])) for o in range(layers[1])]
        acts = [x, np.array(a)]
        for w, b in zip(W[1:], B[1:]):
            a = acts[-1]
            acts.append(np.array([sig(math.fsum([float(w[o, k]) * float(a[k]) for k in range(len(a))] + [float(b[o, 0])]))
                                  for o in range(w.shape[0])]))
        a = acts[-1]
        dl = [(np.asarray(sol, np.float64) - a) * (a * (1.0 - a))]
        for l in range(len(W) - 1, 0, -1):
            nxt, a = dl[0], acts[l]
            s = np.array([math.fsum(float(W[l][o, k]) * float(nxt[o]) for o in range(W[l].shape[0]))
                          for k in range(W[l].shape[1])])
            dl.insert(0, s * (a * (1.0 - a)))
        terms.append((acts, dl))
    Wn, Bn = eo.split(layers, new)
    for acts, dl in terms:
        for l in range(len(Wn)):
            cd = c * dl[l]
            if l == 0:
                x = acts[0]
                Wn[0][:, :8] += np.outer(cd, x[:8])
                Wn[0][:, 8 + np.flatnonzero(x[8:] != 0)] += cd[:, None]
            else:
                Wn[l] += np.outer(cd, acts[l])
            Bn[l][:, 0] += cd
    return new


def worst_rel(got, want):
    """max |got - want| / |want| over the elements that differ (0 when none does)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    m = got != want
    return float(np.max(np.abs(got[m] - want[m]) / np.abs(want[m]))) if m.any() else 0.0


# One step: the project's figure for this kernel family.  Twenty steps: 100 x the worst relative difference of an updated
# weight between `learn` and `learn_exact` after twenty steps, measured by tests/test_population_learn.py (which prints
# both figures and asserts that the numpy model stays 10 x inside each); profiles/r27_population_learn.txt has the run.
RTOL_STEP = 1e-12
MEASURED_20_STEPS = 2.2e-14        # measured 2.165e-14 (one step: 2.219e-14)
RTOL_TRAJECTORY = 100 * MEASURED_20_STEPS

# the trajectory both test files walk: a frozen 48 x 40 scene, the `random` bots' actions at ticks 100 .. 119 as the
# teacher, ship i of arena a on genome (a * M + i) % P
TRAJ = dict(W=48, H=40, M=3, N=2, P=4, seed=5, ticks=6, steps=20, tick0=100, rate=0.5, hidden=(9,))


def trajectory_genomes(layers, n_set):
    """The P genomes the trajectory starts from: evolution_cases.scaled_genome, nothing saturated."""
    from tests import evolution_cases as ec
    rs = np.random.RandomState(27)
    return [ec.scaled_genome(layers, n_set, rs) for _ in range(TRAJ["P"])]


def trajectory_assignment():
    N, M, P = TRAJ["N"], TRAJ["M"], TRAJ["P"]
    return (np.arange(N * M, dtype=np.int32).reshape(N, M)) % P


# ---------------------------------------------------------------- inputs on which a relative tolerance means something
# An updated element is w + t_1 + ... + t_n.  Each term carries the relative error of its sample's deltas, a few ulp
# over the smallest |solution - a_L| of the sample (the subtraction's cancellation), so the element's ABSOLUTE error is
# about that times sum |t_j|.  A relative bound on the element can only be asked where the element has not cancelled:
# the GPU tests therefore take inputs with every |solution - a_L| >= 1/16 and every updated |element| >= sum |t_j| / 8,
# which bounds the element's relative error by 8 * 16 * a few ulp, some 1e-13, under any correct order of summation.
# Both conditions are read off this model alone.
def spaced_solution(layers, genomes, genome_of, alive, obs, solution):
    """`solution` with every entry of a flown ship that lies within 1/16 of the model's output moved 1/4 away from it."""
    sol = np.array(solution, np.float64)
    N, M = genome_of.shape
    for a in range(N):
        for i in range(M):
            p = int(genome_of[a, i])
            if 0 <= p < len(genomes) and alive[a, i]:
                y = activations(layers, genomes[p], obs_vector(obs[a][0][i], obs[a][1], obs[a][2]))[-1]
                near = np.abs(sol[a, i] - y) < 1.0 / 16
                sol[a, i][near] = np.where(y < 0.5, y + 0.25, y - 0.25)[near]
    return sol


def uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, mask, start):
    """The first of start, start / 2, start / 4, ... at which no updated element of the model ends below an eighth of
    the sum of its terms' magnitudes."""
    rate = float(start)
    for _ in range(24):
        travel = [np.zeros_like(g) for g in genomes]
        new, _, _ = learn_population(layers, genomes, genome_of, alive, obs, solution, mask, rate, travel)
        if all((np.abs(n[t > 0]) * 8 >= t[t > 0]).all() for n, t in zip(new, travel)):
            return rate
        rate /= 2
    raise AssertionError("no rate down to %g keeps the updated elements from cancelling" % rate)
