"""Seeded evolution strategies at the training size (profiles/r29_es.txt, profiles/r30_es_optimizer.txt): `--arenas` (4096) arenas x 8 ships, ship 0 of
every arena flown by a member of the ES population around one centre of the reference's [320008, 9, 4], the seven others
by `random` bots.

kernels  HIP events on the handle's stream (ofx_event_record / ofx_event_elapsed), one event pair per call, ONE handle
         that holds the ES centre AND a stored population of `--stored` (512) genomes, on the scene of
         tools/evolution_time.py (same seed, 40 lock-steps of the bots, lasers in flight).  `--repeats` (3) times,
         alternating: a block of `--calls` (50) calls of
           (a) ofx_es_act with member_of[a][0] = a % P at P = `--small` (4096) and at P = `--large` (32768: one member
               per arena and no member twice), and with every evolved ship on the centre (member P: the path without
               Philox);
           (b) ofx_population_act on the stored population, genome_of[a][0] = a % 512: the yardstick;
         (each call = the 1-bit rasteriser and the one forward launch), then (c) one ofx_es_update per P with a weight on
         EVERY pair (the worst case: ties and incomplete pairs are left out by the library).  Reported: us per call
         (mean of each block), the ratio es_act / population_act, the Philox evaluations one es_act makes (per live
         evolved ship: set cells x n1 + 8 n1 + the later layers and biases), ms per update and the Philox evaluations
         per second it reaches (elements x pairs / time).  Beside every ofx_es_update, on the same handle, with the
         same d and in the same block: (d) one ofx_es_step per rule (momentum, Adam) without and with the statistics -
         the same Philox evaluations, 32 / 48 bytes per element instead of 16 - then the update once more and the four steps in
         reverse order (the first call of a block follows the host's work on d, and position in the block shows);
         reported as ms per call and as the ratio to the block's
         first ofx_es_update.
loop     ESRollout at P = `--small`, `--sigma` (0.05), `--lr` (0.1), `--optimizer` (none; momentum or adam) with
         `--weight-decay` (0), `--eval-arenas` (64) arenas on the centre, `--generations` (5) generations of one
         200-lock-step episode each; a host clock around every generation (its lock-steps, the
         restart, the fitness download, pair_weights and the update), ending in a synchronise.  Reported: ms per
         lock-step and arena-steps/s per generation, fitness_log and centre_log, and with an optimizer step_log (the
         sums of squares of the estimate, the step and the centre per generation).  Whether they rise is an observation
         of this run, not something any test holds the code to.
sigma    per-element adaptive sigma against the scalar calls (profiles/r31_es_sigma.txt): one handle with an Adam centre
         and its sigma vector, ship 0 of every arena on member a % P.  Per P (`--small`, `--large`) ONE warmed-up timing
         block, `--repeats` (3) rounds of: `--calls` (50) calls of ofx_es_act, the same of ofx_es_sigma_act, then one
         ofx_es_step (Adam, no statistics), one ofx_es_sigma_step (Adam, no statistics, a d and an s on EVERY pair), and
         the two steps once more in reverse order.  Reported: us per forward, ms per step and the ratios sigma / scalar
         within the block.  `--no-sigma` leaves the two sigma calls out and creates no vector: the same blocks of
         ofx_es_act and ofx_es_step alone, which is what an older build of the library can run (for a comparison of
         these two kernels across builds, and an A/A run of one build for its noise).
         `loop` takes `--adaptive`: ES(sigma_init=`--sigma`, sigma_lr=`--sigma-lr` (0.2)), ESRollout(sigma=None).
queue    the generational loop against ESRollout(auto_reset=True) - per-arena episodes, members from the device-side
         queue (profiles/r32_es_queue.txt): queue()'s docstring has the protocol.  [--members 4096] [--evaluations 1]
         [--poll-every 8] [--sample-every 10] [--event-steps 200]
Each mode prints one JSON line and, with `--out FILE`, appends it to that file.
Usage: python tools/es_time.py kernels|loop|sigma|queue [--arenas 4096] [--small 4096] [--large 32768] [--stored 512] [--calls 50]
                               [--repeats 3] [--generations 5] [--eval-arenas 64] [--optimizer adam|momentum]
                               [--weight-decay 0.005] [--lr 0.1] [--sigma 0.05] [--adaptive] [--sigma-lr 0.2]
                               [--no-sigma] [--out FILE]

One GPU step per process, each under its own time limit, chained so that a failure ends the chain:
    timeout -k 10 400 python tools/es_time.py kernels --out profiles/r29_es.txt \\
    && timeout -k 10 400 python tools/es_time.py loop --out profiles/r29_es.txt"""
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
from ofighters_amd.es import ES, ESRollout
from ofighters_amd.evolution import Population

M, SEED = 8, 0x0F160123
ARENAS = _arg("--arenas", 4096)
LAYERS = [320008, 9, 4]
SIGMA, LR = _arg("--sigma", 0.05), _arg("--lr", 0.1)
STEP_KINDS = [("momentum", nat.ES_RULE_MOMENTUM, False), ("momentum_stats", nat.ES_RULE_MOMENTUM, True),
              ("adam", nat.ES_RULE_ADAM, False), ("adam_stats", nat.ES_RULE_ADAM, True)]
G = sum(LAYERS[i] * LAYERS[i + 1] + LAYERS[i + 1] for i in range(len(LAYERS) - 1))
_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.uint8)


class _Timer:
    def __init__(self, b):
        self.b, self.next_event = b, 0

    def __call__(self, fn, calls):
        """Mean us per call of `calls` calls of fn, one event pair each."""
        e0 = self.next_event
        for j in range(calls):
            self.b.event_record(e0 + 2 * j)
            fn()
            self.b.event_record(e0 + 2 * j + 1)
        self.b.sync()
        self.next_event = e0 + 2 * calls
        return float(np.mean([self.b.event_elapsed(e0 + 2 * j, e0 + 2 * j + 1) for j in range(calls)])) * 1e3


def _assignment(P, centre=False):
    g = np.full((ARENAS, M), -1, np.int32)
    g[:, 0] = P if centre else np.arange(ARENAS) % P
    return DeviceBuffer(g.nbytes).upload(g)


def kernels():
    calls, repeats = _arg("--calls", 50), _arg("--repeats", 3)
    sizes = [_arg("--small", 4096), _arg("--large", 32768)]
    stored = _arg("--stored", 512)
    b = ArenaBatch(ARENAS, M)
    b.spawn_random(SEED)
    b.rollout(["random"] * M, SEED, 0, 40)
    es = ES(b, LAYERS, SEED)
    b.es_opt_create()                                           # the moments, for ofx_es_step beside ofx_es_update
    stats = DeviceBuffer(24)
    pop = Population(b, LAYERS, stored, SEED)
    g = np.full((ARENAS, M), -1, np.int32)
    g[:, 0] = np.arange(ARENAS) % stored
    pop.assign(g)
    b.bot_actions(["random"] * M, SEED, tick=40)
    b.sync()
    members = {P: _assignment(P) for P in sizes}
    centre = _assignment(sizes[0], centre=True)
    timed = _Timer(b)

    def es_act(buf, P):
        return lambda: b.es_act(buf.ptr, P, SIGMA, SEED, 1)

    for P in sizes:                                             # warm-up: the first calls allocate the maps
        timed(es_act(members[P], P), 5)
    timed(es_act(centre, sizes[0]), 5)
    timed(pop.act, 5)
    act_us, centre_us, pop_us = {P: [] for P in sizes}, [], []
    update_ms = {P: [] for P in sizes}
    step_ms = {P: {kind: [] for kind, _, _ in STEP_KINDS} for P in sizes}
    update_again_ms = {P: [] for P in sizes}                    # the update once more behind the steps,
    step_again_ms = {P: {kind: [] for kind, _, _ in STEP_KINDS} for P in sizes}   # then the steps in reverse order
    rs = np.random.RandomState(0)
    generation = 1
    for _ in range(repeats):
        for P in sizes:
            act_us[P].append(round(timed(es_act(members[P], P), calls), 2))
        centre_us.append(round(timed(es_act(centre, sizes[0]), calls), 2))
        pop_us.append(round(timed(pop.act, calls), 2))
        for P in sizes:
            d = rs.uniform(0.01, 1.0, P // 2) * rs.choice([-1.0, 1.0], P // 2)     # a weight on every pair
            gen = generation
            update_ms[P].append(round(timed(lambda: b.es_update(d, LR / (P * SIGMA), SEED, gen), 1) / 1e3, 3))
            for into, kinds in ((step_ms, STEP_KINDS), (step_again_ms, STEP_KINDS[::-1])):
                for kind, rule, with_stats in kinds:
                    step = lambda: b.es_step(d, rule, 1.0 / (P * SIGMA), 0.005, LR, 0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-8,
                                             SEED, gen, stats_ptr=stats.ptr if with_stats else None)
                    into[P][kind].append(round(timed(step, 1) / 1e3, 3))
                if into is step_ms:
                    update_again_ms[P].append(round(timed(lambda: b.es_update(d, LR / (P * SIGMA), SEED, gen), 1) / 1e3, 3))
            generation += 1
    alive = b.get(nat.F_SHIP_ALIVE)[:, 0] != 0
    sm, lm = b.maps_host(nat.MAP_BITS)
    cells = _POPCOUNT[sm].sum(axis=1, dtype=np.int64) + _POPCOUNT[lm].sum(axis=1, dtype=np.int64)
    later = G - LAYERS[0] * LAYERS[1]
    philox_per_act = int((cells[alive] * LAYERS[1]).sum() + int(alive.sum()) * (8 * LAYERS[1] + later))
    pop_mean = float(np.mean(pop_us))
    out = {"what": "kernels", "arenas": ARENAS, "ships": M, "layers": LAYERS, "elements": G, "calls_per_block": calls,
           "sigma": SIGMA, "stored_population": stored, "population_act_us": pop_us, "es_act_centre_us": centre_us,
           "es_act_centre_over_population_act": round(float(np.mean(centre_us)) / pop_mean, 3),
           "evolved_live_ships": int(alive.sum()), "mean_set_cells_per_arena": round(float(cells.mean()), 1),
           "es_act_philox_evaluations": philox_per_act, "sizes": []}
    for P in sizes:
        act_s, upd_s = float(np.mean(act_us[P])) * 1e-6, float(np.mean(update_ms[P])) * 1e-3
        out["sizes"].append({
            "P": P, "es_act_us": act_us[P], "es_act_over_population_act": round(float(np.mean(act_us[P])) / pop_mean, 3),
            "es_act_philox_per_s": round(philox_per_act / act_s, 1),
            "update_ms": update_ms[P], "update_pairs": P // 2, "update_philox_evaluations": G * (P // 2),
            "update_philox_per_s": round(G * (P // 2) / upd_s, 1), "step_ms": step_ms[P],
            "update_again_ms": update_again_ms[P], "step_again_ms": step_again_ms[P],
            "step_over_update": {kind: round(float(np.mean(step_ms[P][kind])) / float(np.mean(update_ms[P])), 4)
                                 for kind, _, _ in STEP_KINDS}})
    b.close()
    return out


def sigma():
    calls, repeats = _arg("--calls", 50), _arg("--repeats", 3)
    sizes = [_arg("--small", 4096), _arg("--large", 32768)]
    adaptive = "--no-sigma" not in sys.argv
    b = ArenaBatch(ARENAS, M)
    b.spawn_random(SEED)
    b.rollout(["random"] * M, SEED, 0, 40)
    ES(b, LAYERS, SEED)
    b.es_opt_create()
    if adaptive:
        b.es_sigma_create(SIGMA)
    b.bot_actions(["random"] * M, SEED, tick=40)
    b.sync()
    timed = _Timer(b)
    rs = np.random.RandomState(0)
    adam = (0.005, LR, 0.9, 1.0 - 0.9, 0.999, 1.0 - 0.999, 1e-8)
    out = {"what": "sigma", "adaptive": adaptive, "arenas": ARENAS, "ships": M, "layers": LAYERS, "elements": G,
           "calls_per_block": calls, "sigma": SIGMA, "sizes": []}
    for P in sizes:
        buf = _assignment(P)
        d = rs.uniform(0.01, 1.0, P // 2) * rs.choice([-1.0, 1.0], P // 2)         # a weight on every pair
        s = rs.uniform(0.01, 1.0, P // 2) * rs.choice([-1.0, 1.0], P // 2)
        kinds = {"es_act": lambda: b.es_act(buf.ptr, P, SIGMA, SEED, 1),
                 "es_step": lambda: b.es_step(d, nat.ES_RULE_ADAM, 1.0 / (P * SIGMA), *adam, SEED, 1)}
        if adaptive:
            kinds["es_sigma_act"] = lambda: b.es_sigma_act(buf.ptr, P, SEED, 1)
            kinds["es_sigma_step"] = lambda: b.es_sigma_step(d, s, nat.ES_RULE_ADAM, 1.0 / P, *adam, 0.2 / P, SIGMA / 64,
                                                             SIGMA * 4, SEED, 1)
        acts = [k for k in ("es_act", "es_sigma_act") if k in kinds]
        steps = [k for k in ("es_step", "es_sigma_step") if k in kinds]
        for k in acts:                                              # warm-up: maps, the pair list's buffers, the clocks
            timed(kinds[k], 5)
        for k in steps:
            timed(kinds[k], 1)
        res = {k: [] for k in kinds}
        for _ in range(repeats):
            for k in acts:
                res[k].append(round(timed(kinds[k], calls), 2))                     # us per forward
            for k in steps + steps[::-1]:
                res[k].append(round(timed(kinds[k], 1) / 1e3, 3))                   # ms per step
        entry = {"P": P, "es_act_us": res["es_act"], "es_step_adam_ms": res["es_step"]}
        if adaptive:
            entry.update({"es_sigma_act_us": res["es_sigma_act"], "es_sigma_step_adam_ms": res["es_sigma_step"],
                          "sigma_act_over_act": round(float(np.mean(res["es_sigma_act"])) / float(np.mean(res["es_act"])), 4),
                          "sigma_step_over_step": round(float(np.mean(res["es_sigma_step"])) / float(np.mean(res["es_step"])), 4)})
        out["sizes"].append(entry)
    b.close()
    return out


def loop():
    P, generations, eval_arenas = _arg("--small", 4096), _arg("--generations", 5), _arg("--eval-arenas", 64)
    optimizer, weight_decay = _arg("--optimizer", "") or None, _arg("--weight-decay", 0.0)
    adaptive = "--adaptive" in sys.argv
    b = ArenaBatch(ARENAS, M)
    kw = dict(sigma_init=SIGMA, sigma_lr=_arg("--sigma-lr", 0.2)) if adaptive else {}
    es = ES(b, LAYERS, SEED, optimizer=optimizer, weight_decay=weight_decay, **kw)
    T = b.cfg.episode_ticks
    roll = ESRollout(b, es, ["random"] * M, SEED, P, None if adaptive else SIGMA, LR, ships=(0,), eval_arenas=eval_arenas,
                     episode_ticks=T, log_steps=optimizer is not None or adaptive)
    roll.run(1)                                                # the episode-end check stands at the head of a lock-step
    ms = []
    for _ in range(generations):
        b.sync()
        t0 = time.perf_counter()
        roll.run(T)
        b.sync()
        ms.append((time.perf_counter() - t0) * 1e3 / T)
    out = {"what": "loop", "arenas": ARENAS, "ships": M, "layers": LAYERS, "P": P, "sigma": SIGMA, "lr": LR,
           "optimizer": optimizer, "weight_decay": weight_decay, "adaptive": adaptive, "eval_arenas": eval_arenas,
           "episode_ticks": T,
           "generations": roll.generation,
           "ms_per_lock_step": [round(x, 4) for x in ms], "mean_ms_per_lock_step": round(float(np.mean(ms)), 4),
           "arena_steps_per_s": round(ARENAS / (float(np.mean(ms)) * 1e-3), 1),
           "complete_pair_members": [w[-1] for w in roll.weight_log],
           "nonzero_pair_weights": [int(np.count_nonzero(w[0])) for w in roll.weight_log],
           "fitness_log_best": [round(f[0], 3) for f in roll.fitness_log],
           "fitness_log_mean": [round(f[1], 3) for f in roll.fitness_log],
           "centre_log": [round(c, 3) for c in roll.centre_log],
           "step_log": [[float("%.6g" % x) for x in t] for t in roll.step_log]}
    b.close()
    return out


def _queue_loop(P, E, generations, eval_arenas, auto_reset, poll_every, sample_every, event_steps):
    """One ESRollout to `generations` generations under a host clock that stops for the samples; see queue()."""
    b = ArenaBatch(ARENAS, M)
    es = ES(b, LAYERS, SEED)
    T = b.cfg.episode_ticks
    roll = ESRollout(b, es, ["random"] * M, SEED, P, SIGMA, LR, ships=(0,), eval_arenas=eval_arenas, episode_ticks=T,
                     episodes_per_generation=E, **(dict(auto_reset=True, poll_every=poll_every) if auto_reset else {}))
    learn = ARENAS - eval_arenas
    alive, flying, seconds, steps = [], [], 0.0, 0
    b.sync()
    t0 = time.perf_counter()
    while roll.generation < generations:
        roll.lockstep()
        steps += 1
        if steps % sample_every == 0:                           # the clock stops for the sample
            b.sync()
            seconds += time.perf_counter() - t0
            a = b.get(nat.F_SHIP_ALIVE)[:learn, 0] != 0
            if auto_reset:                                      # an idle ship (member -1, the tail) evaluates nothing
                held = es.member_of_host()[:learn, 0] >= 0
                a &= held
                flying.append(float(held.mean()))
            alive.append(float(a.mean()))
            t0 = time.perf_counter()
    b.sync()
    seconds += time.perf_counter() - t0
    if auto_reset:
        evaluations = sum(g[1] for g in roll.generation_log)
        per_generation = [g[0] for g in roll.generation_log]
    else:
        evaluations = generations * E * learn                   # every learning arena's ship banks once per episode
        per_generation = [E * T] * generations
    out = {"auto_reset": auto_reset, "P": P, "E": E, "generations": roll.generation, "lock_steps": steps,
           "lock_steps_per_generation": per_generation, "seconds": round(seconds, 4),
           "ms_per_lock_step": round(seconds * 1e3 / steps, 4), "member_evaluations": int(evaluations),
           "member_evaluations_per_s": round(evaluations / seconds, 1),
           "members_of_complete_pairs": [w[-1] for w in roll.weight_log],
           "share_evaluating_at_forward": round(float(np.mean(alive)), 4), "samples": len(alive),
           "fitness_log_mean": [round(f[1], 3) for f in roll.fitness_log],
           "centre_log": [round(c, 3) for c in roll.centre_log]}
    if auto_reset:
        out["share_holding_a_ticket"] = round(float(np.mean(flying)), 4)
        out["centre_episodes_per_generation"] = [g[2] for g in roll.generation_log]
        # restart_finished + requeue at the head of `event_steps` more lock-steps, one event pair each
        e, rf, rq, j = roll.e, roll.e.restart_finished, es.requeue, [0]

        def restart_finished(*a, **k):
            e.event_record(2 * j[0])
            return rf(*a, **k)

        def requeue(bank=True):
            rq(bank)
            if bank:
                e.event_record(2 * j[0] + 1)
                j[0] += 1
        e.restart_finished, es.requeue = restart_finished, requeue
        g0 = roll.generation
        while j[0] < event_steps and roll.generation == g0:
            roll.lockstep()
        e.restart_finished, es.requeue = rf, rq
        b.sync()
        us = [b.event_elapsed(2 * i, 2 * i + 1) * 1e3 for i in range(j[0])]
        out["restart_finished_plus_requeue_us"] = {"lock_steps": j[0], "mean": round(float(np.mean(us)), 2),
                                                   "median": round(float(np.median(us)), 2),
                                                   "max": round(float(np.max(us)), 2)}
    b.close()
    return out


def queue():
    """`queue`: the old generational loop against ESRollout(auto_reset=True) (profiles/r32_es_queue.txt) at P =
    `--members` (4096), E = `--evaluations` (1), `--generations` (3), `--eval-arenas` (64), `--poll-every` (8).  A host
    clock around the lock-steps of each loop, ending in a synchronise and stopped for the samples: every
    `--sample-every` (10) lock-steps, the share of the learning arenas' evolved ships that are alive and fly a member.
    Then, with the option on, `--event-steps` (200) lock-steps with one event pair around restart_finished + requeue."""
    P, E, generations = _arg("--members", 4096), _arg("--evaluations", 1), _arg("--generations", 3)
    args = (P, E, generations, _arg("--eval-arenas", 64))
    rest = (_arg("--poll-every", 8), _arg("--sample-every", 10), _arg("--event-steps", 200))
    return {"what": "queue", "arenas": ARENAS, "ships": M, "layers": LAYERS, "sigma": SIGMA, "lr": LR,
            "old": _queue_loop(*args, False, *rest), "new": _queue_loop(*args, True, *rest)}


if __name__ == "__main__":
    what = [x for x in sys.argv[1:] if x in ("kernels", "loop", "sigma", "queue")]
    if len(what) != 1:
        raise SystemExit(__doc__)
    line = json.dumps({"kernels": kernels, "loop": loop, "sigma": sigma, "queue": queue}[what[0]]())
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(_arg("--out", ""), "a") as f:
            f.write(line + "\n")
