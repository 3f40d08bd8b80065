"""The learning step per genome at the training size (profiles/r27_population_learn.txt): `--arenas` (4096) arenas x 8
ships, ship 0 of every arena flown by a genome of the reference's [320008, 9, 4], the seven others by `random` bots.

kernels  HIP events on the handle's stream, one event pair per call, two handles in ONE process - `--small` (512)
         genomes on one, `--large` (4096) on the other - on the same arenas (same seed, 40 lock-steps of the bots).
         `--repeats` (3) times, alternating blocks of `--calls` (50) calls of
           (a) ofx_population_act;
           (b) ofx_population_learn at rate 2^-10 toward the bots' own actions (ofx_population_targets once, before);
           (c) ofx_population_learn at rate 0: the rasteriser and phase A alone, so (b) - (c) is phase B.
         Reported: us per call, learn / act, phase B's share, and the algorithmic bytes of (b): the set cells of the
         samples' arenas x n1 x 16 B read-modify-write plus the two bit maps twice.
act      ofx_population_act alone on the small population, `--repeats` blocks of `--calls` calls; with `--lib FILE` on
         another build of the library (the parent commit's), so that two builds alternate as PROCESSES.
loop     EvolutionRollout on the small population, `--generations` (4) generations of one 200-lock-step episode: the
         first half with imitate_rate 2^-10 (the imitation lock-step), the second half plain; a host clock around every
         generation.  Reported: ms per lock-step of each, imitation_log, fitness_log - observations of one run.
Each mode prints one JSON line and, with `--out FILE`, appends it to that file.

One GPU step per process, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 400 python tools/population_learn_time.py kernels --out profiles/r27_population_learn.txt \\
    && timeout -k 10 200 python tools/population_learn_time.py act --out profiles/r27_population_learn.txt \\
    && timeout -k 10 400 python tools/population_learn_time.py loop --out profiles/r27_population_learn.txt"""
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

from ofighters_amd import _native as nat

LIB = _arg("--lib", "")
if LIB:                                   # another build: bind what it exports (an older one lacks the newest entries)
    nat.LIB_PATH = os.path.abspath(LIB)
    _probe = C.CDLL(nat.LIB_PATH)
    for _name in [n for n in nat.SIGNATURES if not hasattr(_probe, n)]:
        del nat.SIGNATURES[_name]

from ofighters_amd import ArenaBatch, DeviceBuffer
from ofighters_amd.evolution import EvolutionRollout, Population

M, SEED = 8, 0x0F160123
ARENAS = _arg("--arenas", 4096)
LAYERS = [320008, 9, 4]
RATE = 2.0 ** -10
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


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
        self.us = {"act": [], "learn": [], "phase_a": []}

    def targets(self):
        nm = ARENAS * M
        self.sol, self.mask = DeviceBuffer(nm * 32), DeviceBuffer(nm)
        self.b.population_targets(self.sol.ptr, self.mask.ptr)
        self.b.sync()

    def learn(self, rate):
        self.pop.learn(self.sol.ptr, rate, mask_ptr=self.mask.ptr)

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

    def learn_bytes(self):
        """Algorithmic bytes of one learn call: per sample, set cells x n1 x 16 and the two bit maps twice."""
        alive = self.b.get(nat.F_SHIP_ALIVE)[:, 0] != 0
        valid = self.b.actions_host()["valid"][:, 0] != 0
        sample = alive & valid
        sm, lm = self.b.maps_host(nat.MAP_BITS)
        cells = _POPCOUNT[sm].sum(axis=1, dtype=np.int64) + _POPCOUNT[lm].sum(axis=1, dtype=np.int64)
        maps = 2 * sm.shape[1]
        return (int((cells[sample] * LAYERS[1] * 16).sum() + 2 * maps * int(sample.sum())), int(sample.sum()),
                float(cells.mean()))


def kernels():
    calls, repeats = _arg("--calls", 50), _arg("--repeats", 3)
    sides = [_Side(_arg("--small", 512)), _Side(_arg("--large", 4096))]
    for s in sides:
        nbytes = s.learn_bytes()
        s.targets()
        s.bytes = nbytes
        s.timed(s.pop.act, 5)                                   # warm-up: the first calls allocate the maps, the workspace
        s.timed(lambda: s.learn(RATE), 5)
    for _ in range(repeats):
        for s in sides:
            s.us["act"].append(round(s.timed(s.pop.act, calls), 2))
            s.us["learn"].append(round(s.timed(lambda: s.learn(RATE), calls), 2))
            s.us["phase_a"].append(round(s.timed(lambda: s.learn(0.0), calls), 2))
    out = {"what": "kernels", "arenas": ARENAS, "ships": M, "layers": LAYERS, "calls_per_block": calls, "rate": RATE,
           "populations": []}
    for s in sides:
        act, learn, pa = (float(np.mean(s.us[k])) for k in ("act", "learn", "phase_a"))
        nbytes, samples, cells = s.bytes
        out["populations"].append({
            "P": s.P, "act_us": s.us["act"], "learn_us": s.us["learn"], "learn_rate0_us": s.us["phase_a"],
            "learn_over_act": round(learn / act, 3), "phase_b_share": round((learn - pa) / learn, 3),
            "samples": samples, "mean_set_cells_per_arena": round(cells, 1), "learn_algorithmic_bytes": nbytes,
            "learn_algorithmic_bytes_per_s": round(nbytes / (learn * 1e-6), 1)})
        s.b.close()
    return out


def act():
    calls, repeats = _arg("--calls", 50), _arg("--repeats", 3)
    s = _Side(_arg("--small", 512))
    s.timed(s.pop.act, 5)
    us = [round(s.timed(s.pop.act, calls), 2) for _ in range(repeats)]
    s.b.close()
    return {"what": "act", "lib": LIB or "this build", "arenas": ARENAS, "P": s.P, "calls_per_block": calls, "act_us": us}


def loop():
    P, generations = _arg("--small", 512), _arg("--generations", 4)
    b = ArenaBatch(ARENAS, M)
    pop = Population(b, LAYERS, P, SEED)
    T = b.cfg.episode_ticks
    roll = EvolutionRollout(b, pop, ["random"] * M, SEED, ships=(0,), survivors=max(1, P // 4), dafts=P // 8,
                            episode_ticks=T, imitate_rate=RATE, imitate_generations=generations // 2)
    roll.run(1)                                                # the episode-end check stands at the head of a lock-step
    ms = []
    for _ in range(generations):
        b.sync()
        t0 = time.perf_counter()
        roll.run(T)
        b.sync()
        ms.append(round((time.perf_counter() - t0) * 1e3 / T, 4))
    h = generations // 2
    out = {"what": "loop", "arenas": ARENAS, "ships": M, "layers": LAYERS, "P": P, "episode_ticks": T,
           "imitate_rate": RATE, "imitate_generations": h, "ms_per_lock_step": ms,
           "imitation_ms_per_lock_step": round(float(np.mean(ms[:h])), 4),
           "plain_ms_per_lock_step": round(float(np.mean(ms[h:])), 4),
           "imitation_log": [(g, round(e, 3), n) for g, e, n in roll.imitation_log],
           "fitness_log_best": [round(f[0], 3) for f in roll.fitness_log],
           "fitness_log_mean": [round(f[1], 3) for f in roll.fitness_log]}
    b.close()
    return out


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("kernels", "act", "loop")]
    if len(what) != 1:
        raise SystemExit(__doc__)
    line = json.dumps({"kernels": kernels, "act": act, "loop": loop}[what[0]]())
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", ""), "a") as f:
            f.write(line + "\n")
