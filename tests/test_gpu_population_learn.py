"""ofx_population_learn / ofx_population_targets on the GPU against tests/learn_oracle.py (numpy float64, the contract of
include/ofx.h): forward outputs bit for bit, every element of every genome, the untouched cells, the order of the
samples, the imitation trajectory, the loop with its checkpoint, the refusals."""
import os

import numpy as np
import pytest

from tests import evolution_cases as ec
from tests import learn_oracle as lo

pytestmark = pytest.mark.gpu

SEED = 0x0E7090FF
RATE = 0.5            # where the halving of lo.uncancelled_rate starts
SENTINEL = -7.25


def _flat(pop, p):
    w, b = pop.b.population_get(p, pop.n_weights, pop.n_biases)
    return np.concatenate([w, b])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assignment(N, M, P):
    """-1s, one genome on two ships of an arena, the same genome in two arenas; (N-1, 1) is the ship that gets killed;
    slot P - 2 is on nobody."""
    g = np.full((N, M), -1, np.int32)
    g[0, 0], g[0, 1] = P - 1, P - 1
    g[1, 0], g[1, 1], g[1, 2] = P - 1, 0, 1
    g[2, 1], g[2, 2], g[2, M - 1] = 1, 3, 2
    return g


def _scene(b, SEED):
    """Crafted start: in the last arena ship 2 shoots ship 1 (destroyed on the second lock-step), then four lock-steps
    of the random bots put lasers in flight everywhere."""
    from ofighters_amd import pack_actions, _native as nat
    N, M = b.N, b.M
    b.spawn_random(SEED)
    x, y = b.get(nat.F_SHIP_X).copy(), b.get(nat.F_SHIP_Y).copy()
    sx, sy, vx, vy = 8, b.H // 2, 30, b.H // 2
    x[N - 1, 2], y[N - 1, 2], x[N - 1, 1], y[N - 1, 1] = sx, sy, vx, vy
    b.set_ships(x=x, y=y, px=x, py=y)
    z = np.zeros((N, M), np.int32)
    valid, shoot, px, py = z.copy(), z.copy(), z.copy(), z.copy()
    valid[N - 1, 2], shoot[N - 1, 2], px[N - 1, 2], py[N - 1, 2] = 1, 1, vx, vy
    b.step(actions=pack_actions(valid, shoot, z, px, py))
    b.step(actions=pack_actions(z, z, z, z, z))
    assert b.get(nat.F_SHIP_ALIVE)[N - 1, 1] == 0, "the crafted shot did not destroy its target"
    for t in range(4):
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.step()


def _observations(b):
    """(obs[a] = (head [M][8], ship_map, laser_map), alive [N][M]) as the device holds them."""
    from ofighters_amd import _native as nat
    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_F64)
    return [(head[a], sm[a], lm[a]) for a in range(b.N)], b.get(nat.F_SHIP_ALIVE) != 0


def _population(b, layers, genomes, genome_of):
    """A fresh population on b holding `genomes` (element vectors)."""
    from ofighters_amd.evolution import Population
    pop = Population(b, layers, len(genomes), SEED, init=False)
    nw = pop.n_weights
    for p, g in enumerate(genomes):
        b.population_set(p, g[:nw], g[nw:])
    pop.assign(genome_of)
    return pop


def _learn(b, pop, solution, mask, rate):
    """One learn call with sentinel-filled outputs: (y, err, actions after, genomes after)."""
    from ofighters_amd import DeviceBuffer
    N, M = b.N, b.M
    dy = DeviceBuffer(N * M * 32).upload(np.full((N, M, 4), SENTINEL))
    de = DeviceBuffer(N * M * 8).upload(np.full((N, M), SENTINEL))
    ds = DeviceBuffer(N * M * 32).upload(np.ascontiguousarray(solution, np.float64))
    dm = None if mask is None else DeviceBuffer(N * M).upload(np.ascontiguousarray(mask, np.uint8))
    pop.learn(ds.ptr, rate, mask_ptr=None if dm is None else dm.ptr, y_ptr=dy.ptr, err_ptr=de.ptr)
    b.sync()
    return (dy.download(np.float64, (N, M, 4)), de.download(np.float64, (N, M)), b.actions_host(),
            [_flat(pop, p) for p in range(pop.P)])


def _check_against_model(layers, genomes, genome_of, alive, obs, solution, mask, rate, got, err, tag=""):
    """Every element of every genome within RTOL_STEP of the model; untouched first-layer cells and sample-less genomes
    keep their bits; err of the samples within RTOL_STEP, of the others the sentinel."""
    want, want_err, _ = lo.learn_population(layers, genomes, genome_of, alive, obs, solution, mask, rate)
    nin, n1 = layers[0], layers[1]
    worst = 0.0
    for p, (old, new, w) in enumerate(zip(genomes, got, want)):
        samples = [(a, i) for (a, i) in want_err if genome_of[a, i] == p]
        worst = max(worst, lo.worst_rel(new, w))
        print("%s genome %d: worst relative difference %.3e" % (tag, p, lo.worst_rel(new, w)))
        np.testing.assert_allclose(new, w, rtol=lo.RTOL_STEP, atol=0, err_msg="%s genome %d" % (tag, p))
        if not samples:
            assert np.array_equal(_bits(new), _bits(old)), "%s genome %d has no sample and changed" % (tag, p)
            continue
        assert not np.array_equal(new, old)
        seen = np.zeros(nin - 8, bool)
        for a, _ in samples:
            seen |= np.concatenate([obs[a][1].ravel(), obs[a][2].ravel()]) != 0
        first_old, first_new = old[:nin * n1].reshape(n1, nin)[:, 8:], new[:nin * n1].reshape(n1, nin)[:, 8:]
        assert np.array_equal(_bits(first_old[:, ~seen]), _bits(first_new[:, ~seen])), "%s genome %d: an unset cell" % (tag, p)
        assert (first_old[:, seen] != first_new[:, seen]).any()
    N, M = genome_of.shape
    for a in range(N):
        for i in range(M):
            if (a, i) in want_err:
                np.testing.assert_allclose(err[a, i], want_err[a, i], rtol=lo.RTOL_STEP, atol=0)
            else:
                assert err[a, i] == SENTINEL
    print("%s: rate %g, worst relative difference of an element %.3e, %d samples" % (tag, rate, worst, len(want_err)))
    return want_err


CONTRACT = [(W, H, M, hidden) for (W, H) in ((48, 40), (80, 52)) for M in (3, 13) for hidden in ((9,), (13, 7))]


@pytest.mark.parametrize("W,H,M,hidden", CONTRACT)
def test_learn_contract(W, H, M, hidden):
    from ofighters_amd import ArenaBatch, DeviceBuffer
    N, P = 3, 6
    layers = [8 + 2 * W * H] + list(hidden) + [4]
    b = ArenaBatch(N, M, width=W, height=H)
    _scene(b, SEED)
    obs, alive = _observations(b)
    rs = np.random.RandomState(W + M + len(hidden))
    n_set = len(ec.set_cells(obs[0][1], obs[0][2]))
    genomes = [ec.scaled_genome(layers, n_set, rs) for _ in range(P)]
    genome_of = _assignment(N, M, P)
    solution = lo.spaced_solution(layers, genomes, genome_of, alive, obs, rs.uniform(0.05, 0.95, (N, M, 4)))
    mask = np.ones((N, M), np.uint8)
    mask[0, 1] = 0                                        # assigned, alive, masked out; its genome has other samples
    rate = lo.uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, mask, RATE)
    assert not alive[N - 1, 1] and genome_of[N - 1, 1] >= 0 and alive[0, 1] and not (genome_of == P - 2).any()

    pop = _population(b, layers, genomes, genome_of)
    b.bot_actions(["random"] * M, SEED, tick=100)
    before = b.actions_host()
    dy = DeviceBuffer(N * M * 32).upload(np.full((N, M, 4), SENTINEL))
    pop.act(y_ptr=dy.ptr)
    b.sync()
    y_act, a_act = dy.download(np.float64, (N, M, 4)), b.actions_host()
    b.bot_actions(["random"] * M, SEED, tick=100)          # the acting call's entries are overwritten again
    assert b.actions_host().tobytes() == before.tobytes()

    y, err, actions, got = _learn(b, pop, solution, mask, rate)
    # the forward outputs are the acting call's, bit for bit - for the masked-out ship too; the others are not written
    assert np.array_equal(_bits(y), _bits(y_act)) and actions.tobytes() == a_act.tobytes()
    assert (y[0, 1] != SENTINEL).all() and (y[N - 1, 1] == SENTINEL).all()
    want_err = _check_against_model(layers, genomes, genome_of, alive, obs, solution, mask, rate, got, err,
                                    "%dx%d M=%d %s" % (W, H, M, hidden))
    assert (0, 1) not in want_err and (0, 0) in want_err and (1, 0) in want_err
    pop.close()

    # a second population set to the same genomes: the same bits
    pop = _population(b, layers, genomes, genome_of)
    y2, err2, _, got2 = _learn(b, pop, solution, mask, rate)
    assert np.array_equal(_bits(y2), _bits(y)) and np.array_equal(_bits(err2), _bits(err))
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(got, got2))
    pop.close()

    # a NULL mask is all ones
    pop = _population(b, layers, genomes, genome_of)
    _, err_ones, _, got_ones = _learn(b, pop, solution, np.ones((N, M), np.uint8), rate)
    pop.close()
    pop = _population(b, layers, genomes, genome_of)
    _, err_null, _, got_null = _learn(b, pop, solution, None, rate)
    assert np.array_equal(_bits(err_ones), _bits(err_null)) and err_null[0, 1] != SENTINEL
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(got_ones, got_null))
    assert not np.array_equal(got_null[P - 1], got[P - 1])
    pop.close()

    # rate = 0: outputs and err, no genome bit
    pop = _population(b, layers, genomes, genome_of)
    y0, err0, _, got0 = _learn(b, pop, solution, mask, 0.0)
    assert np.array_equal(_bits(y0), _bits(y)) and np.array_equal(_bits(err0), _bits(err))
    assert all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(genomes, got0))
    b.close()


@pytest.mark.parametrize("hidden", [(1,), (33,), (64,), ()], ids=["n1=1", "n1=33", "n1=64", "no-hidden"])
def test_learn_lane_layouts(hidden):
    from ofighters_amd import ArenaBatch
    W, H, M, N, P = 24, 20, 3, 2, 2
    layers = [8 + 2 * W * H] + list(hidden) + [4]
    b = ec.scene(W, H, M, 34, 6).device(N)
    obs, alive = _observations(b)
    rs = np.random.RandomState(len(hidden) + sum(hidden))
    genomes = [ec.scaled_genome(layers, len(ec.set_cells(obs[0][1], obs[0][2])), rs) for _ in range(P)]
    genome_of = (np.arange(N * M, dtype=np.int32).reshape(N, M)) % P
    solution = lo.spaced_solution(layers, genomes, genome_of, alive, obs, rs.uniform(0.05, 0.95, (N, M, 4)))
    rate = lo.uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, None, RATE)
    pop = _population(b, layers, genomes, genome_of)
    _, err, _, got = _learn(b, pop, solution, None, rate)
    _check_against_model(layers, genomes, genome_of, alive, obs, solution, None, rate, got, err, "24x20 %s" % (hidden,))
    b.close()


def test_learn_through_the_flush():
    """The dense case of tests/evolution_cases.py: a wave's list flushes twice inside the update's walk."""
    W, H, M, N, P = 128, 128, 64, 1, 2
    layers = [8 + 2 * W * H, 9, 4]
    b = ec.scene(W, H, M, 5, 0).device(N)
    obs, alive = _observations(b)
    assert max(ec.quarter_counts(obs[0][1], obs[0][2])) > 2 * ec.POP_LIST
    rs = np.random.RandomState(128)
    genomes = [ec.scaled_genome(layers, len(ec.set_cells(obs[0][1], obs[0][2])), rs) for _ in range(P)]
    genome_of = np.full((N, M), -1, np.int32)
    genome_of[0, 3], genome_of[0, 40], genome_of[0, 17] = 1, 1, 0     # one genome on two ships of the arena
    assert alive[0, 3] and alive[0, 40] and alive[0, 17]
    solution = lo.spaced_solution(layers, genomes, genome_of, alive, obs, rs.uniform(0.05, 0.95, (N, M, 4)))
    rate = lo.uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, None, RATE)
    pop = _population(b, layers, genomes, genome_of)
    _, err, _, got = _learn(b, pop, solution, None, rate)
    _check_against_model(layers, genomes, genome_of, alive, obs, solution, None, rate, got, err, "dense 128x128")
    b.close()


def test_learn_more_samples_than_one_list_pass():
    """384 ships on one genome: the update's sample list is filled more than once, and the order is the contract's."""
    from ofighters_amd import ArenaBatch
    W, H, N, M, P = 16, 8, 48, 8, 2
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(N, M, width=W, height=H)
    b.spawn_random(SEED)
    obs, alive = _observations(b)
    assert alive.all()
    rs = np.random.RandomState(384)
    genomes = [ec.scaled_genome(layers, len(ec.set_cells(obs[0][1], obs[0][2])), rs) for _ in range(P)]
    genome_of = np.zeros((N, M), np.int32)
    solution = lo.spaced_solution(layers, genomes, genome_of, alive, obs, rs.uniform(0.05, 0.95, (N, M, 4)))
    rate = lo.uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, None, 8.0)   # c = rate / 384
    pop = _population(b, layers, genomes, genome_of)
    _, err, _, got = _learn(b, pop, solution, None, rate)
    want_err = _check_against_model(layers, genomes, genome_of, alive, obs, solution, None, rate, got, err, "384 samples")
    assert len(want_err) == 384 and np.array_equal(_bits(got[1]), _bits(genomes[1]))
    b.close()


def test_learn_at_full_size():
    from ofighters_amd import ArenaBatch
    W, H, N, M, P = 400, 400, 2, 3, 2
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(N, M, width=W, height=H)
    b.spawn_random(SEED)
    for t in range(4):
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.step()
    obs, alive = _observations(b)
    rs = np.random.RandomState(400)
    genomes = [ec.scaled_genome(layers, len(ec.set_cells(obs[0][1], obs[0][2])), rs) for _ in range(P)]
    genome_of = np.array([[0, 1, -1], [1, 1, 0]], np.int32)
    solution = lo.spaced_solution(layers, genomes, genome_of, alive, obs, rs.uniform(0.05, 0.95, (N, M, 4)))
    rate = lo.uncancelled_rate(layers, genomes, genome_of, alive, obs, solution, None, RATE)
    pop = _population(b, layers, genomes, genome_of)
    _, err, _, got = _learn(b, pop, solution, None, rate)
    _check_against_model(layers, genomes, genome_of, alive, obs, solution, None, rate, got, err, "400x400")
    b.close()


def test_imitation_trajectory():
    """Twenty imitate steps on a frozen scene against the `random` bots' actions at fixed ticks: err per step within the
    tolerance tests/test_population_learn.py derives (100 x the model's own twenty-step deviation from its exact twin)."""
    from ofighters_amd import DeviceBuffer
    T = lo.TRAJ
    W, H, M, N, P = T["W"], T["H"], T["M"], T["N"], T["P"]
    layers = [8 + 2 * W * H] + list(T["hidden"]) + [4]
    b = ec.scene(W, H, M, T["seed"], T["ticks"]).device(N)
    obs, alive = _observations(b)
    genomes = lo.trajectory_genomes(layers, len(ec.set_cells(obs[0][1], obs[0][2])))
    genome_of = lo.trajectory_assignment()
    pop = _population(b, layers, genomes, genome_of)
    de = DeviceBuffer(N * M * 8)
    model = [g.copy() for g in genomes]
    first = last = None
    for t in range(T["steps"]):
        b.bot_actions(["random"] * M, T["seed"], tick=T["tick0"] + t)
        teacher = b.actions_host()
        de.upload(np.full((N, M), SENTINEL))
        pop.imitate(T["rate"], err_ptr=de.ptr)
        b.sync()
        err = de.download(np.float64, (N, M))
        sol, mask = np.zeros((N, M, 4)), np.zeros((N, M), bool)
        for a in range(N):
            for i in range(M):
                tc = teacher[a, i]
                sol[a, i], mask[a, i] = lo.targets((tc["valid"], tc["shoot"], tc["thrust"], tc["px"], tc["py"]), W, H)
        model, want_err, want_y = lo.learn_population(layers, model, genome_of, alive, obs, sol, mask, T["rate"])
        after = b.actions_host()
        for a in range(N):
            for i in range(M):
                if (a, i) in want_err:
                    np.testing.assert_allclose(err[a, i], want_err[a, i], rtol=lo.RTOL_TRAJECTORY, atol=0,
                                               err_msg="step %d ship (%d, %d)" % (t, a, i))
                    assert after[a, i]["valid"] == 1       # the student flies: its own decoded action stands there
                else:
                    assert err[a, i] == SENTINEL
                    if not alive[a, i] or genome_of[a, i] < 0:
                        assert after[a, i].tobytes() == teacher[a, i].tobytes()
        total = sum(want_err.values())
        first, last = (total if first is None else first), total
        print("step %2d: %d samples, summed err device %.12f model %.12f" % (t, len(want_err), np.sum(err[err != SENTINEL]), total))
    for p in range(P):
        print("genome %d after %d steps: worst relative difference %.3e" % (p, T["steps"], lo.worst_rel(_flat(pop, p), model[p])))
    for p in range(P):
        np.testing.assert_allclose(_flat(pop, p), model[p], rtol=lo.RTOL_TRAJECTORY, atol=0)
    b.close()


def _rollout(seed, stop_at=None, tmp=None):
    """2 generations of 2 episodes of 6 lock-steps, imitation in the first; with stop_at: stopped there, saved, restored
    into fresh handles and continued."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import EvolutionRollout, Population
    N, M, P, W, H, T = 4, 3, 4, 48, 40, 6
    layers = [8 + 2 * W * H, 9, 4]
    total = 4 * T + 1

    def make():
        b = ArenaBatch(N, M, width=W, height=H)
        pop = Population(b, layers, P, seed)
        roll = EvolutionRollout(b, pop, ["random"] * M, seed, ships=(0, 2), survivors=2, dafts=1, episode_ticks=T,
                                episodes_per_generation=2, imitate_rate=0.5, imitate_generations=1)
        return b, pop, roll

    b, pop, roll = make()
    if stop_at is not None:
        roll.run(stop_at)
        path = os.path.join(tmp, "population.npy")
        pop.save(path)
        state = roll.state_dict()
        b.close()
        b, pop, roll = make()
        pop.load(path)
        roll.load_state_dict(state)
        roll.run(total - stop_at)
    else:
        roll.run(total)
    out = dict(genomes=[_flat(pop, p) for p in range(P)], fitness_log=list(roll.fitness_log),
               imitation_log=list(roll.imitation_log), plans=[p.copy() for p in roll.plans],
               score_log=[s.copy() for s in roll.score_log], state=b.state_dict(), generation=roll.generation,
               fitness=pop.fitness_host())
    b.close()
    return out


def test_loop_and_resume(tmp_path):
    whole = _rollout(SEED)
    assert whole["generation"] == 2 and [e[0] for e in whole["imitation_log"]] == [0, 0]
    assert all(n > 0 and err > 0 for _, err, n in whole["imitation_log"])
    for stop_at in (9, 15):                               # mid-episode under imitation; mid-generation after it
        part = _rollout(SEED, stop_at, str(tmp_path))
        for u, v in zip(whole["genomes"], part["genomes"]):
            assert np.array_equal(_bits(u), _bits(v))
        assert whole["fitness_log"] == part["fitness_log"] and whole["imitation_log"] == part["imitation_log"]
        assert whole["generation"] == part["generation"]
        assert all(np.array_equal(u, v) for u, v in zip(whole["plans"], part["plans"]))
        assert all(np.array_equal(u, v) for u, v in zip(whole["score_log"], part["score_log"]))
        assert all(np.array_equal(u, v) for u, v in zip(whole["fitness"], part["fitness"]))
        assert sorted(whole["state"]) == sorted(part["state"]) and len(whole["state"]) == 19 + 2
        for k, v in whole["state"].items():
            assert np.array_equal(v, part["state"][k]), k


def test_population_load_refuses(tmp_path):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import Population
    W, H = 16, 8
    b = ArenaBatch(1, 1, width=W, height=H)
    pop = Population(b, [8 + 2 * W * H, 3, 4], 2, SEED)
    path = pop.save(str(tmp_path / "p.npy"))
    want = [_flat(pop, p) for p in range(2)]
    pop.close()
    for layers, P, seed, field in (([8 + 2 * W * H, 4, 4], 2, SEED, "layers"), ([8 + 2 * W * H, 3, 4], 3, SEED, "P"),
                                   ([8 + 2 * W * H, 3, 4], 2, SEED + 1, "seed")):
        other = Population(b, layers, P, seed)
        with pytest.raises(ValueError, match=field):
            other.load(path)
        other.close()
    again = Population(b, [8 + 2 * W * H, 3, 4], 2, SEED, init=False)
    again.load(path)
    assert all(np.array_equal(_bits(_flat(again, p)), _bits(want[p])) for p in range(2))
    b.close()


def test_learn_refusals():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    W, H = 16, 8
    b = ArenaBatch(1, 2, width=W, height=H)
    b.spawn_random(SEED)
    g = DeviceBuffer(8).upload(np.zeros(2, np.int32))
    sol = DeviceBuffer(64).upload(np.zeros(8))
    with pytest.raises(OfxError, match="no population") as e:
        b.population_learn(g.ptr, sol.ptr, 0.1)
    assert e.value.code == nat.OFX_ERR_STATE
    b.population_create([8 + 2 * W * H, 3, 4], 1)
    b.population_init(SEED)
    for args, word in (((g.ptr, sol.ptr, float("nan")), "finite"), ((g.ptr, sol.ptr, float("inf")), "finite"),
                       ((g.ptr, None, 0.1), "NULL"), ((None, sol.ptr, 0.1), "NULL")):
        with pytest.raises(OfxError, match=word) as e:
            b.population_learn(*args)
        assert e.value.code == nat.OFX_ERR_INVALID
    with pytest.raises(OfxError) as e:
        b.population_targets(None, None)
    assert e.value.code == nat.OFX_ERR_INVALID
    b.population_learn(g.ptr, sol.ptr, 0.1, actions=False)   # actions, y, err and the mask may all be NULL
    b.sync()
    b.close()
