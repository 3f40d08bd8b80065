"""Neuroevolution at the training size (profiles/r23_evolution.txt): `--arenas` (4096) arenas x 8 ships, ship 0 of every
arena flown by a genome of the reference's [320008, 9, 4], the seven others by `random` bots.

kernels  HIP events on the handle's stream (ofx_event_record / ofx_event_elapsed), one event pair per call, two handles
         in ONE process - a population of `--small` (512) genomes on one, of `--large` (4096, 94 GB) on the other - on
         the same arenas (same seed, 40 lock-steps of the bots, lasers in flight).  `--repeats` (3) times, alternating:
         a block of `--calls` (50) calls of
           (a) ofx_population_act on the small population, then on the large one (each call = the 1-bit rasteriser and
               the one forward launch), genome_of[a][0] = a % P;
           (b) ofx_scratch_feed_obs, the shared-weights yardstick, on the first handle (the rasteriser and its launches),
               and ofx_rasterise(OFX_MAP_BITS) alone: the 1-bit rasteriser both of them start with;
         then (c) one ofx_population_breed per population on a truncation-shaped plan (P/4 kept, P/8 fresh, the rest
         children dealt round-robin).  Reported: us per call (mean of each block), the algorithmic bytes - for (a) the
         set cells of the evolved live ships' arenas x n1 x 8 plus their two bit maps, for (c) one genome written per
         rewritten slot plus one read per child - and the fraction of the 8 TB/s HBM specification they reach.
loop     (d), (e): EvolutionRollout on the small population, survivors P/4, dafts P/8, `--generations` (30) generations of
         one 200-lock-step episode each; a host clock around every generation (its lock-steps, the restart, the fitness
         download, the plan and the breed), ending in a synchronise.  Reported: ms per lock-step and arena-steps/s per
         generation, and fitness_log (best genome's mean score, mean score per evolved ship).  Whether the fitness rises
         is an observation of this run, not something any test holds the code to.
Each mode prints one JSON line and, with `--out FILE`, appends it to that file.
Usage: python tools/evolution_time.py kernels|loop [--arenas 4096] [--small 512] [--large 4096] [--calls 50]
                                      [--repeats 3] [--generations 30] [--out FILE]

One GPU step per process, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 400 python tools/evolution_time.py kernels --out profiles/r23_evolution.txt \\
    && timeout -k 10 400 python tools/evolution_time.py loop --out profiles/r23_evolution.txt"""
import ctypes as C
import json
import os
import sys
import time


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
from ofighters_amd.evolution import EvolutionRollout, Population, truncation_plan

M, SEED, HBM_SPEC = 8, 0x0F160123, 8.0e12
ARENAS = _arg("--arenas", 4096)
LAYERS = [320008, 9, 4]
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


def _plan(P):
    """The shape truncation selection gives: P/4 kept, P/8 fresh, the others children."""
    return truncation_plan(np.arange(P, 0, -1, dtype=np.int64), np.ones(P, np.int32), max(1, P // 4), P // 8)


class _Side:
    def __init__(self, P):
        self.P = P
        self.b = ArenaBatch(ARENAS, M)
        self.b.spawn_random(SEED)
        self.b.rollout(["random"] * M, SEED, 0, 40)
        self.pop = Population(self.b, LAYERS, P, SEED)
        g = np.full((ARENAS, M), -1, np.int32)
        g[:, 0] = np.arange(ARENAS) % P
        self.pop.assign(g)
        self.b.bot_actions(["random"] * M, SEED, tick=40)
        self.next_event = 0
        self.act_us, self.breed_ms = [], []

    def timed(self, fn, calls):
        """Mean us per call of `calls` calls of fn, one event pair each."""
        e0 = self.next_event
        for j in range(calls):
            self.b.event_record(e0 + 2 * j)
            fn()
            self.b.event_record(e0 + 2 * j + 1)
        self.b.sync()
        self.next_event = e0 + 2 * calls
        return float(np.mean([self.b.event_elapsed(e0 + 2 * j, e0 + 2 * j + 1) for j in range(calls)])) * 1e3

    def act_bytes(self):
        """Algorithmic bytes of one ofx_population_act: per evolved live ship, set cells x n1 x 8 and the two bit maps."""
        alive = self.b.get(nat.F_SHIP_ALIVE)[:, 0] != 0
        sm, lm = self.b.maps_host(nat.MAP_BITS)
        cells = _POPCOUNT[sm].sum(axis=1, dtype=np.int64) + _POPCOUNT[lm].sum(axis=1, dtype=np.int64)
        maps = 2 * sm.shape[1]
        return int((cells[alive] * LAYERS[1] * 8).sum() + maps * int(alive.sum())), int(alive.sum()), float(cells.mean())


def kernels():
    calls, repeats = _arg("--calls", 50), _arg("--repeats", 3)
    sides = [_Side(_arg("--small", 512)), _Side(_arg("--large", 4096))]
    first = sides[0]
    rs = np.random.RandomState(0)
    w = 2 * rs.random_sample(LAYERS[0] * LAYERS[1] + LAYERS[1] * LAYERS[2]) - 1
    bb = 2 * rs.random_sample(LAYERS[1] + LAYERS[2]) - 1
    dw, db = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(bb.nbytes).upload(bb)
    dy = DeviceBuffer(8 * ARENAS * M * 4)
    larr = np.asarray(LAYERS, np.int32)
    lp = larr.ctypes.data_as(C.c_void_p)

    def feed():
        nat.check(nat.lib().ofx_scratch_feed_obs(first.b.handle, lp, 3, dw.ptr, db.ptr, dy.ptr, None))

    for s in sides:                                             # warm-up: the first calls allocate the maps
        s.timed(s.pop.act, 5)
    first.timed(feed, 5)
    first.timed(lambda: first.b.rasterise(nat.MAP_BITS), 5)
    feed_us, raster_us, generation = [], [], 0
    for _ in range(repeats):
        for s in sides:
            s.act_us.append(round(s.timed(s.pop.act, calls), 2))
        feed_us.append(round(first.timed(feed, calls), 2))
        raster_us.append(round(first.timed(lambda: first.b.rasterise(nat.MAP_BITS), calls), 2))
        generation += 1
        for s in sides:
            g = generation
            s.breed_ms.append(round(s.timed(lambda: s.pop.breed(_plan(s.P), 0.05, 0.05, g), 1) / 1e3, 3))
    G = LAYERS[0] * LAYERS[1] + LAYERS[1] * LAYERS[2] + LAYERS[1] + LAYERS[2]
    out = {"what": "kernels", "arenas": ARENAS, "ships": M, "layers": LAYERS, "calls_per_block": calls,
           "scratch_feed_obs_us": feed_us, "rasterise_bits_us": raster_us, "hbm_spec_bytes_per_s": HBM_SPEC, "populations": []}
    for s in sides:
        nbytes, live, cells = s.act_bytes()
        plan = _plan(s.P)
        children = int(((plan >= 0) & (plan != np.arange(s.P))).sum())
        fresh = int((plan == -1).sum())
        breed_bytes = (2 * children + fresh) * G * 8
        act_s, breed_s = float(np.mean(s.act_us)) * 1e-6, float(np.mean(s.breed_ms)) * 1e-3
        out["populations"].append({
            "P": s.P, "population_bytes": s.P * G * 8, "act_us": s.act_us, "evolved_live_ships": live,
            "mean_set_cells_per_arena": round(cells, 1), "act_algorithmic_bytes": nbytes,
            "act_fraction_of_hbm_spec": round(nbytes / act_s / HBM_SPEC, 4),
            "breed_ms": s.breed_ms, "breed_children": children, "breed_fresh": fresh,
            "breed_algorithmic_bytes": breed_bytes, "breed_fraction_of_hbm_spec": round(breed_bytes / breed_s / HBM_SPEC, 4)})
    for s in sides:
        s.b.close()
    return out


def loop():
    P, generations = _arg("--small", 512), _arg("--generations", 30)
    b = ArenaBatch(ARENAS, M)
    pop = Population(b, LAYERS, P, SEED)
    T = b.cfg.episode_ticks
    roll = EvolutionRollout(b, pop, ["random"] * M, SEED, ships=(0,), survivors=max(1, P // 4), dafts=P // 8,
                            episode_ticks=T)
    roll.run(1)                                                # the episode-end check stands at the head of a lock-step
    ms = []
    for _ in range(generations):
        b.sync()
        t0 = time.perf_counter()
        roll.run(T)
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / T)
    out = {"what": "loop", "arenas": ARENAS, "ships": M, "layers": LAYERS, "P": P, "survivors": roll.survivors,
           "dafts": roll.dafts, "evolution_rate": roll.evolution_rate, "mutation_rate": roll.mutation_rate,
           "episode_ticks": T, "generations": roll.generation,
           "ms_per_lock_step": [round(x, 4) for x in ms], "mean_ms_per_lock_step": round(float(np.mean(ms)), 4),
           "arena_steps_per_s": round(ARENAS / (float(np.mean(ms)) * 1e-3), 1),
           "fitness_log_best": [round(f[0], 3) for f in roll.fitness_log],
           "fitness_log_mean": [round(f[1], 3) for f in roll.fitness_log]}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("kernels", "loop")]
    if len(what) != 1:
        raise SystemExit(__doc__)
    line = json.dumps(kernels() if what[0] == "kernels" else loop())
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", ""), "a") as f:
            f.write(line + "\n")
