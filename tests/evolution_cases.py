"""Scenes, genomes and the exactly rounded reference of tests/test_evolution_edges.py (CPU: the preconditions, the
tolerance and its power) and tests/test_gpu_evolution_edges.py (GPU: the same cases on the device).  A helper module
(not collected).

The cases aim at the branches of k_pop_act (ofx_evolve.hip; its walk and forward are ofx_genome.h's) that a sparse,
even-sized map never takes: the mid-walk flush of a wave's cell list, the ship/laser boundary inside one wave's span, and the lane layouts n1 = 1 .. 64."""
import math

import numpy as np

from tests import evolution_oracle as eo

POP_LIST = 2048                      # ofx_genome.h: set cells one wave lists before it gathers
BEHAVIOURS = ("shoot", "turret")     # the bots of a scene with ticks > 0, dealt round-robin over the ships
P = 5                                # genomes of a forward case
RTOL = 1e-12                         # the project's figure for this kernel family; test_evolution_edges.py shows per
                                     # case that the numpy reference stays within a tenth of it, 1e-13, of the exact one

# (kind, W, H, M, hidden, ticks, seed).  The seeds are those at which arena 0 meets the kind's precondition
# (tests/test_evolution_edges.py asserts it):
#   "dense"  a ship-map quarter lists more than 2 * POP_LIST cells: the flush fires at least twice
#   "odd"    an odd number of map words, and set cells on both sides of the ship/laser boundary inside wave 1's span
#   "one"    one word per map, every cell set: waves 2 and 3 own nothing
#   "plain"  neither: the case is about the layers
# A quarter of a 96 x 96 ship map holds 4608 cells and 48 ships set about 2900 of them: one flush, not two.  The second
# dense shape is therefore 160 x 120 with 64 ships (4844 cells in quarter 0, 2243 in quarter 1: wave 1 flushes once).
FORWARD_CASES = [
    ("dense", 128, 128, 64, (13, 7), 0, 5),
    ("dense", 128, 128, 64, (64,), 0, 5),
    ("dense", 128, 128, 64, (1,), 0, 5),
    ("dense", 160, 120, 64, (9,), 0, 5),
    ("odd", 56, 36, 5, (33,), 6, 14),
    ("odd", 56, 36, 5, (63,), 6, 14),
    ("odd", 24, 20, 3, (32,), 6, 34),
    ("one", 8, 4, 1, (9,), 0, 5),
    ("plain", 48, 40, 3, (), 6, 5),
    ("plain", 48, 40, 3, (64,) * 6, 6, 5),
]
# rtol of a case whose numpy reference does not stay within RTOL / 10 of the exact one: ten times the measured
# deviation, the figure beside it.  None so far: the worst case measures 6.2e-15.
CASE_RTOL = {}


def case_id(case):
    kind, W, H, M, hidden, _, _ = case
    return "%s-%dx%d-M%d-%s" % (kind, W, H, M, "x".join(map(str, hidden)) or "none")


def case_layers(case):
    _, W, H, _, hidden, _, _ = case
    return [8 + 2 * W * H] + list(hidden) + [4]


def case_rtol(case):
    return CASE_RTOL.get(case_id(case), RTOL)


class Scene:
    """One arena content, buildable on both sides: spawn `seed`, then `ticks` lock-steps of the BEHAVIOURS bots."""

    def __init__(self, W, H, M, seed, ticks=0):
        self.W, self.H, self.M, self.seed, self.ticks = W, H, M, seed, ticks
        self.behaviours = [BEHAVIOURS[i % len(BEHAVIOURS)] for i in range(M)]

    def oracle(self, N=1, arena_base=0):
        """The CPU side: an EvolutionOracleBatch of N arenas (pyoracle.Arena each), global ids from arena_base."""
        b = eo.EvolutionOracleBatch(N, self.M, self.W, self.H, arena_base)
        b.spawn_random(self.seed)
        for t in range(self.ticks):
            b.bot_actions(self.behaviours, self.seed, tick=t)
            b.step()
        return b

    def device(self, N=1, arena_base=0):
        """The GPU side: an ArenaBatch spawned and stepped the same way, as tests/test_gpu_step.py does."""
        from ofighters_amd import ArenaBatch
        b = ArenaBatch(N, self.M, width=self.W, height=self.H, arena_base=arena_base)
        b.spawn_random(self.seed)
        for t in range(self.ticks):
            b.bot_actions(self.behaviours, self.seed, tick=t)
            b.step()
        return b


def scene(W, H, M, seed, ticks=0):
    """What both sides need to build the same arena: .oracle(N) on the CPU, .device(N) on the GPU."""
    return Scene(W, H, M, seed, ticks)


def case_scene(case):
    _, W, H, M, _, ticks, seed = case
    return Scene(W, H, M, seed, ticks)


def observation(arena):
    """(head [M][8], ship_map, laser_map, alive [M]) of one pyoracle.Arena."""
    sm, lm = arena.rasterise()
    head, _ = arena.obs_head()
    return head, sm, lm, arena.ships()["alive"]


def set_cells(ship_map, laser_map):
    """Indices of the set cells in toVector's run [ship_map.ravel() | laser_map.ravel()], ascending."""
    return np.flatnonzero(np.concatenate([np.asarray(ship_map).ravel(), np.asarray(laser_map).ravel()]) != 0)


def quarter_counts(ship_map, laser_map):
    """Set cells in each quarter [q * per, min(total, (q + 1) * per)) of the run of total = 2 * words 32-cell words,
    per = ceil(total / 4).

    This mirrors k_pop_act's split of the two bit maps over its four waves (pop_walk in ofx_genome.h: `per = (total + 3) / 4`)
    and is read against POP_LIST, a copy of that file's constant: it must move with them."""
    cells = np.asarray(ship_map).size
    assert cells % 32 == 0
    words = cells // 32
    total, per = 2 * words, (2 * words + 3) // 4
    at = set_cells(ship_map, laser_map) // 32
    return [int(((at >= q * per) & (at < min(total, (q + 1) * per))).sum()) for q in range(4)]


def scaled_genome(layers, n_set, rs):
    """An element vector whose every element is +-U[0.25, 1), the map columns of the first layer times 1/sqrt(n_set)
    and its eight head columns times 1 / (4 * sqrt(W * H)).

    No weight is near zero, so a dropped or doubled cell always shows; the sum over about n_set map cells has a
    standard deviation near 0.66 and the head (coordinates up to max(W, H)) adds about as much, so the first layer's
    pre-activations stay O(1) and nothing saturates and hides it."""
    g = rs.uniform(0.25, 1.0, eo.n_elements(layers)) * rs.choice([-1.0, 1.0], eo.n_elements(layers))
    W, _ = eo.split(layers, g)
    W[0][:, :8] *= 1.0 / (4.0 * math.sqrt((layers[0] - 8) / 2))
    W[0][:, 8:] *= 1.0 / math.sqrt(max(int(n_set), 1))
    return g


def _sigmoid(z):
    return 1.0 / (1.0 + math.exp(-z))


def first_layer_exact(layers, g, head8, ship_map, laser_map, drop=None, extra=None):
    """The first layer's pre-activations (bias included), every sum by math.fsum.  drop / extra: one cell index of
    the 2 * W * H run that is removed from / added to the listed set cells (it must be set / clear)."""
    W, B = eo.split(layers, np.asarray(g, np.float64))
    cells = set_cells(ship_map, laser_map)
    if drop is not None:
        assert drop in cells
        cells = cells[cells != drop]
    if extra is not None:
        assert extra not in cells
        cells = np.sort(np.append(cells, extra))
    head = [float(v) for v in head8]
    return [math.fsum([float(W[0][o, k]) * head[k] for k in range(8)] + W[0][o, 8 + cells].tolist() + [float(B[0][o, 0])])
            for o in range(layers[1])]


def forward_exact(layers, g, head8, ship_map, laser_map, drop=None, extra=None):
    """evolution_oracle.forward with every dot product (products rounded once, bias included) summed by math.fsum,
    which is exactly rounded: the high-precision reference."""
    W, B = eo.split(layers, np.asarray(g, np.float64))
    a = [_sigmoid(z) for z in first_layer_exact(layers, g, head8, ship_map, laser_map, drop, extra)]
    for w, b in zip(W[1:], B[1:]):
        a = [_sigmoid(math.fsum([float(w[o, k]) * a[k] for k in range(len(a))] + [float(b[o, 0])]))
             for o in range(w.shape[0])]
    return np.array(a)


def assignment(case, N):
    """genome_of (int32 [N][M]) of a forward case: about eight ships of an arena fly, genome (a * M + i) % P, and every
    fourth of those stays unassigned.  The dead are assigned like the living: the device must leave them alone."""
    M = case[3]
    stride = max(1, M // 8)
    g = np.full((N, M), -1, np.int32)
    for a in range(N):
        for i in range(0, M, stride):
            if (a + i // stride) % 4 != 3:
                g[a, i] = (a * M + i) % P
    return g


def genomes_for(case, n_set):
    """The P scaled genomes of a forward case, seeded by its shape."""
    _, W, H, M, hidden, _, _ = case
    rs = np.random.RandomState(1000 * len(hidden) + sum(hidden) + W + M)
    layers = case_layers(case)
    return [scaled_genome(layers, n_set, rs) for _ in range(P)]


def rel_dev(got, want):
    """max |got - want| / |want| over the outputs."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


# the breed of more jobs than the grid has rows: a 16 x 8 arena, 273 elements, and the slots both test files sample
# around the 65 535 rows and at the end of 70 000
BREED_LAYERS = [8 + 2 * 16 * 8, 1, 4]
BREED_SLOTS = [0, 1, 65534, 65535, 65536, 65537, 69999]

N_ARENAS = 3
_REFERENCES = {}


def case_reference(case):
    """What both test files hold a forward case to, from the oracle alone and computed once: the observations of the
    N_ARENAS arenas, the assignment, the genomes, and forward_exact of every flown (assigned and alive) ship."""
    key = case_id(case)
    if key not in _REFERENCES:
        M, layers = case[3], case_layers(case)
        obs = [observation(a) for a in case_scene(case).oracle(N_ARENAS).arenas]
        genomes = genomes_for(case, len(set_cells(obs[0][1], obs[0][2])))
        genome_of = assignment(case, N_ARENAS)
        exact = {}
        for a, (head, sm, lm, alive) in enumerate(obs):
            for i in range(M):
                if genome_of[a, i] >= 0 and alive[i]:
                    exact[a, i] = forward_exact(layers, genomes[genome_of[a, i]], head[i], sm, lm)
        _REFERENCES[key] = dict(layers=layers, obs=obs, genomes=genomes, genome_of=genome_of, exact=exact)
    return _REFERENCES[key]
