"""Neuroevolution of the scratch MLP on the GPU: the forward with a genome per ship, reproduction, 64-bit offsets,
fitness and the generational loop, each against tests/evolution_oracle.py (numpy float64, the contract of include/ofx.h)."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import evolution_oracle as eo

pytestmark = pytest.mark.gpu

SEED = 0x0E7090FF


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _flat(pop, p):
    """Slot p of a Population as one element vector, through ofx_population_get."""
    w, b = pop.b.population_get(p, pop.n_weights, pop.n_biases)
    return np.concatenate([w, b])


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _assignment(N, M, P):
    """-1s, one genome on two ships of an arena, the same genome in two arenas; (N-1, 1) is the ship that gets killed."""
    g = np.full((N, M), -1, np.int32)
    g[0, 0], g[0, 1] = P - 1, P - 1
    g[1, 0], g[1, 1], g[1, 2] = P - 1, 0, 1 % P
    if N > 2:
        g[2, 1], g[2, 2], g[2, M - 1] = 1 % P, 3 % P, 2 % P
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


def _scaled_genome(layers, rs):
    """Weights that keep the first layer's pre-activations O(1): the outputs are then far from saturation and the
    comparison sees every term of the sum."""
    g = rs.uniform(-1, 1, eo.n_elements(layers))
    W, B = eo.split(layers, g.copy())
    W[0][:, :8] *= 0.01
    W[0][:, 8:] *= 0.05
    return W, B


FORWARD_CASES = [(48, 40, M, hidden) for M in (3, 13) for hidden in ((9,), (13, 7))] + \
                [(80, 52, M, hidden) for M in (3, 13) for hidden in ((9,), (13, 7))] + [(400, 400, 3, (9,))]


@pytest.mark.parametrize("W,H,M,hidden", FORWARD_CASES)
def test_forward_with_a_genome_per_ship(W, H, M, hidden):
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.evolution import Population
    big = W == 400
    N, P = (2, 2) if big else (3, 5)
    layers = [8 + 2 * W * H] + list(hidden) + [4]
    b = ArenaBatch(N, M, width=W, height=H)
    _scene(b, SEED)
    pop = Population(b, layers, P, SEED)
    rs = np.random.RandomState(3)
    for p in range(1, P, 2):                              # the odd slots through `set`, the others are init's
        pop.set_genome(p, *_scaled_genome(layers, rs))
    genome_of = _assignment(N, M, P)
    pop.assign(genome_of)
    b.bot_actions(["random"] * M, SEED, tick=100)
    before = b.actions_host()
    sentinel = np.full((N, M, 4), -7.25)
    dy = DeviceBuffer(sentinel.nbytes).upload(sentinel)
    pop.act(y_ptr=dy.ptr)
    b.sync()
    y, after = dy.download(np.float64, (N, M, 4)), b.actions_host()
    pop.act(y_ptr=dy.ptr)
    b.sync()
    assert np.array_equal(_bits(y), _bits(dy.download(np.float64, (N, M, 4)))), "a second call gives other bits"
    assert after.tobytes() == b.actions_host().tobytes()

    alive = b.get(nat.F_SHIP_ALIVE)
    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_F64)
    flown = (genome_of >= 0) & (alive != 0)
    assert not flown[N - 1, 1] and genome_of[N - 1, 1] >= 0 and flown.sum() >= 3
    genomes = {int(p): _flat(pop, int(p)) for p in np.unique(genome_of[flown])}
    # the same exported genome through ofx_scratch_feed_obs (shared weights, another summation order)
    shared = {}
    larr = np.asarray(layers, np.int32)
    dys = DeviceBuffer(8 * N * M * 4)
    for p, g in genomes.items():
        nw = pop.n_weights
        dw, db = DeviceBuffer(8 * nw).upload(g[:nw]), DeviceBuffer(8 * pop.n_biases).upload(g[nw:])
        nat.check(nat.lib().ofx_scratch_feed_obs(b.handle, _vp(larr), len(layers), dw.ptr, db.ptr, dys.ptr, None))
        b.sync()
        shared[p] = dys.download(np.float64, (N, M, 4))
    for a in range(N):
        for i in range(M):
            if not flown[a, i]:
                # dead, unassigned: neither y nor the action is written
                assert np.array_equal(y[a, i], sentinel[a, i])
                assert after[a, i].tobytes() == before[a, i].tobytes()
                continue
            p = int(genome_of[a, i])
            want = eo.forward(layers, genomes[p], head[a, i], sm[a], lm[a])
            print("case %dx%d M=%d %s arena %d ship %d genome %d: max rel err numpy %.3e, scratch_feed_obs %.3e"
                  % (W, H, M, hidden, a, i, p, np.max(np.abs(y[a, i] - want) / np.abs(want)),
                     np.max(np.abs(y[a, i] - shared[p][a, i]) / np.abs(shared[p][a, i]))))
            np.testing.assert_allclose(y[a, i], want, rtol=1e-12, atol=0)
            np.testing.assert_allclose(y[a, i], shared[p][a, i], rtol=1e-12, atol=0)
            d = eo.decode(y[a, i], W, H)                 # the decode of the device's own y, exactly
            got = after[a, i]
            assert [got["valid"], got["shoot"], got["thrust"], got["px"], got["py"], got["_pad"]] == list(d) + [0]
    # one genome on two ships of an arena and in two arenas: the same weights, other observations
    assert genome_of[0, 0] == genome_of[0, 1] == genome_of[1, 0]
    b.close()


RATES = [(0.05, 0.05), (0.0, 0.3), (0.3, 0.0)]


@pytest.mark.parametrize("evo,mut", RATES)
def test_reproduction_bit_for_bit(evo, mut):
    from ofighters_amd import ArenaBatch, _native as nat
    from ofighters_amd.evolution import Population
    W, H, P = 48, 40, 7
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(1, 1, width=W, height=H)
    pop = Population(b, layers, P, SEED)
    want = [eo.fresh(layers, SEED, p, 0) for p in range(P)]
    for p in range(P):
        assert np.array_equal(_bits(_flat(pop, p)), _bits(want[p])), "init, slot %d" % p
    # `set` then `get` round-trips, -0.0 and a denormal included
    rs = np.random.RandomState(8)
    g = rs.uniform(-1, 1, eo.n_elements(layers))
    g[:3] = [-0.0, 5e-324, 1.0]
    pop.set_genome(2, *eo.split(layers, g))
    assert np.array_equal(_bits(_flat(pop, 2)), _bits(g))
    want[2] = g
    # two generations in a row: keep, breed, refresh
    for generation, plan in ((1, [0, 0, -1, 3, 3, 0, -1]), (2, [4, 1, 1, -1, 4, 4, 6])):
        plan = np.asarray(plan, np.int32)
        pop.breed(plan, evo, mut, generation)
        want = eo.breed(want, plan, evo, mut, SEED, generation, layers)
        for p in range(P):
            assert np.array_equal(_bits(_flat(pop, p)), _bits(want[p])), "generation %d, slot %d" % (generation, p)
    # an invalid plan (given to the library itself) is refused with nothing written
    for bad in ([1, 2, 2, 3, 4, 5, 6], [0, 1, 2, 3, 4, 5, 7], [0, 1, 2, 3, 4, 5, -2], [-1, 0, 2, 3, 4, 5, 6]):
        bad = np.asarray(bad, np.int32)
        rc = nat.lib().ofx_population_breed(b.handle, _vp(bad), evo, mut, SEED, 3)
        assert rc == nat.OFX_ERR_INVALID and b"plan[" in nat.lib().ofx_last_error()
        with pytest.raises(ValueError):
            pop.breed(bad, evo, mut, 3)
    for p in range(P):
        assert np.array_equal(_bits(_flat(pop, p)), _bits(want[p])), "after the refused plans, slot %d" % p
    b.close()


def test_population_create_refusals():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    b = ArenaBatch(1, 1, width=48, height=40)
    nin = 8 + 2 * 48 * 40
    for layers, P, word in (([nin + 1, 9, 4], 2, "8 + 2*W*H"), ([nin, 9, 3], 2, "4 outputs"), ([nin, 65, 4], 2, "wide"),
                            ([nin] + [5] * 7 + [4], 2, "layers"), ([nin, 9, 4], 0, "P must")):
        with pytest.raises(OfxError) as e:
            b.population_create(layers, P)
        assert e.value.code == nat.OFX_ERR_INVALID and word in str(e.value)
    with pytest.raises(OfxError, match="no population"):
        b.population_init(1)
    with pytest.raises(OfxError, match="bytes") as e:      # 4 TB cannot be allocated: the message names the bytes
        b.population_create([nin, 64, 64, 4], 2000000)
    assert e.value.code == nat.OFX_ERR_HIP and str(2000000 * eo.n_elements([nin, 64, 64, 4]) * 8) in str(e.value)
    b.population_create([nin, 9, 4], 2)
    with pytest.raises(OfxError, match="already"):
        b.population_create([nin, 9, 4], 2)
    b.population_destroy()
    b.population_create([nin, 9, 4], 3)
    b.close()                                              # ofx_destroy frees it


def _free_hbm():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def test_offsets_past_2_31_elements():
    """P x elements passes 2^31 at slot 746 of the reference's size: slots on both sides of it and the last one."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import Population
    P, layers = 760, [320008, 9, 4]
    b = ArenaBatch(1, 1)
    need = P * eo.n_elements(layers) * 8
    free = _free_hbm()
    if free < need + (1 << 30):
        b.close()
        pytest.skip("the device reports %.1f GB free, the population needs %.1f GB" % (free / 1e9, need / 1e9))
    pop = Population(b, layers, P, SEED)
    plan = np.arange(P, dtype=np.int32)
    plan[759] = 0
    pop.breed(plan, 0.05, 0.05, 1)
    for p in (0, 745, 746):
        assert np.array_equal(_bits(_flat(pop, p)), _bits(eo.fresh(layers, SEED, p, 0))), "slot %d" % p
    want = eo.child(eo.fresh(layers, SEED, 0, 0), SEED, 759, 1, 0.05, 0.05)
    assert np.array_equal(_bits(_flat(pop, 759)), _bits(want)), "slot 759"
    b.close()


def test_fitness_sums():
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.evolution import Population
    N, M, P, W, H = 5, 4, 6, 48, 40
    b = ArenaBatch(N, M, width=W, height=H)
    b.spawn_random(SEED)
    pop = Population(b, [8 + 2 * W * H, 9, 4], P, SEED)
    rs = np.random.RandomState(2)
    genome_of = rs.randint(-1, P - 1, (N, M)).astype(np.int32)     # slot P - 1 is flown by nobody
    pop.assign(genome_of)
    want_s, want_c = np.zeros(P, np.int64), np.zeros(P, np.int32)
    tick = 0
    for episode in range(3):
        for _ in range(12):
            b.bot_actions(["shoot", "random", "turret", "random"], SEED, tick=tick)
            pop.act()
            b.step()
            tick += 1
        b.restart_random(SEED)
        pop.fitness(reset=episode == 1)                  # the second episode starts the sums again, the third adds
        last = b.get(nat.F_LAST_SCORES)
        if episode == 1:
            want_s[:], want_c[:] = 0, 0
        for g in range(P):
            want_s[g] += int(last[genome_of == g].sum())
            want_c[g] += int((genome_of == g).sum())
        s, c = pop.fitness_host()
        assert s.dtype == np.int64 and c.dtype == np.int32
        assert np.array_equal(s, want_s) and np.array_equal(c, want_c), "episode %d" % episode
    assert want_s.any() and want_c[P - 1] == 0
    b.close()


def _loop(seed):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import EvolutionRollout, Population
    N, M, P, W, H, T = 8, 3, 4, 48, 40, 10
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(N, M, width=W, height=H)
    pop = Population(b, layers, P, seed)
    roll = EvolutionRollout(b, pop, ["random"] * M, seed, ships=(0,), survivors=2, dafts=1, episode_ticks=T)
    snaps = [[_flat(pop, p) for p in range(P)]]
    for _ in range(3):
        roll.run(T + (1 if len(snaps) == 1 else 0))      # up to and including the lock-step that ends a generation
        snaps.append([_flat(pop, p) for p in range(P)])
    out = dict(fitness_log=list(roll.fitness_log), plans=[p.copy() for p in roll.plans], snaps=snaps,
               generation=roll.generation, assignment=pop.genome_of.copy(), want_assignment=roll.assignment(3))
    b.close()
    return out


def test_evolution_loop_on_the_device():
    r1, r2 = _loop(SEED), _loop(SEED)
    assert r1["generation"] == 3 and len(r1["fitness_log"]) == 3 and len(r1["plans"]) == 3
    assert r1["fitness_log"] == r2["fitness_log"]
    for s1, s2 in zip(r1["snaps"], r2["snaps"]):
        for g1, g2 in zip(s1, s2):
            assert np.array_equal(_bits(g1), _bits(g2))
    assert np.array_equal(r1["assignment"], r1["want_assignment"])
    # survivors are bit-unchanged across a generation; everything else follows the oracle's breed
    layers = [8 + 2 * 48 * 40, 9, 4]
    for gen, plan in enumerate(r1["plans"]):
        old, new = r1["snaps"][gen], r1["snaps"][gen + 1]
        kept = np.flatnonzero(plan == np.arange(len(plan)))
        assert len(kept) == 2
        for p in kept:
            assert np.array_equal(_bits(old[p]), _bits(new[p]))
        want = eo.breed(old, plan, 0.05, 0.05, SEED, gen + 1, layers)
        for p in range(len(plan)):
            assert np.array_equal(_bits(new[p]), _bits(want[p])), "generation %d, slot %d" % (gen + 1, p)
    assert not np.array_equal(r1["snaps"][0][int(np.flatnonzero(r1["plans"][0] == -1)[0])],
                              r1["snaps"][1][int(np.flatnonzero(r1["plans"][0] == -1)[0])])
