"""The evolved-ship forward, breeding and fitness where tests/test_gpu_evolution.py does not reach: dense maps (the
mid-walk flush of k_pop_act's cell lists), an odd number of map words (the ship/laser boundary inside one wave's span),
first layers 1 to 64 wide, 2 and 8 layers, more breeding jobs than the grid has rows, scores of either sign; and the
scratch-MLP forward the first is cross-checked against, at the widths and depths its own test leaves out.

The forward cases, their exactly rounded reference and the tolerance come from tests/evolution_cases.py;
tests/test_evolution_edges.py shows on the CPU that each scene takes its branch, that the numpy reference meets the
tolerance with a factor of ten to spare and that one lost or doubled cell misses it a thousandfold."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from tests import evolution_cases as ec
from tests import evolution_oracle as eo
from tests.evolution_cases import BREED_LAYERS, BREED_SLOTS

pytestmark = pytest.mark.gpu

SEED = 0x0E7090FF
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _flat(pop, p):
    w, b = pop.b.population_get(p, pop.n_weights, pop.n_biases)
    return np.concatenate([w, b])


def _assert_scene(b, obs):
    """The device's arenas hold what the oracle's do: alive flags, observation heads and both maps, exactly."""
    from ofighters_amd import _native as nat
    alive = b.get(nat.F_SHIP_ALIVE)
    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_U8)
    for a, (ohead, osm, olm, oalive) in enumerate(obs):
        assert np.array_equal(alive[a], oalive) and np.array_equal(head[a], ohead), "arena %d" % a
        assert np.array_equal(sm[a], osm) and np.array_equal(lm[a], olm), "arena %d" % a


def _population(b, layers, genomes):
    from ofighters_amd.evolution import Population
    pop = Population(b, layers, len(genomes), SEED, init=False)
    for p, g in enumerate(genomes):
        pop.set_genome(p, *eo.split(layers, g))
    return pop


def _act(b, pop, raw_genome_of, sentinel=-7.25):
    """ofx_population_act on a genome_of written to the device as it is (Population.assign refuses out-of-range
    values): (y [N][M][4] over a sentinel, the action array after the call)."""
    from ofighters_amd import DeviceBuffer
    N, M = b.N, b.M
    b.sync()
    pop._genome_of.upload(np.ascontiguousarray(raw_genome_of, np.int32))
    dy = DeviceBuffer(8 * N * M * 4).upload(np.full((N, M, 4), sentinel))
    b.population_act(pop._genome_of.ptr, y_ptr=dy.ptr)
    b.sync()
    return dy.download(np.float64, (N, M, 4)), b.actions_host()


def _feed_obs(b, layers, weights, biases, want_argmax=False):
    """ofx_scratch_feed_obs on flat host weights: y [N][M][layers[-1]] (and the argmax [N][M])."""
    from ofighters_amd import DeviceBuffer, _native as nat
    N, M, larr = b.N, b.M, np.asarray(layers, np.int32)
    assert weights.size == sum(layers[i] * layers[i + 1] for i in range(len(layers) - 1)) and biases.size == sum(layers[1:])
    dw, db = DeviceBuffer(weights.nbytes).upload(weights), DeviceBuffer(biases.nbytes).upload(biases)
    dy, da = DeviceBuffer(8 * N * M * layers[-1]), DeviceBuffer(4 * N * M)
    nat.check(nat.lib().ofx_scratch_feed_obs(b.handle, _vp(larr), len(layers), dw.ptr, db.ptr, dy.ptr, da.ptr))
    b.sync()
    y = dy.download(np.float64, (N, M, layers[-1]))
    return (y, da.download(np.int32, (N, M))) if want_argmax else y


@pytest.mark.parametrize("case", ec.FORWARD_CASES, ids=ec.case_id)
def test_forward_at_dense_maps_and_odd_shapes(case):
    kind, W, H, M, hidden, ticks, seed = case
    ref = ec.case_reference(case)
    layers, rtol, N = ref["layers"], ec.case_rtol(case), ec.N_ARENAS
    b = ec.case_scene(case).device(N)
    _assert_scene(b, ref["obs"])
    pop = _population(b, layers, ref["genomes"])
    # two ships nobody flies are named out of range: the contract leaves them alone like the unassigned
    genome_of = ref["genome_of"]
    raw = genome_of.copy()
    free = np.argwhere(genome_of < 0)
    if kind != "one":
        assert len(free) >= 2
        raw[tuple(free[0])], raw[tuple(free[-1])] = ec.P, INT32_MAX
    b.bot_actions(["random"] * M, seed, tick=100)
    before = b.actions_host()
    y, after = _act(b, pop, raw)
    y2, after2 = _act(b, pop, raw)
    assert np.array_equal(_bits(y), _bits(y2)) and after.tobytes() == after2.tobytes(), "a second call gives other bits"

    nw = pop.n_weights
    shared = {p: _feed_obs(b, layers, g[:nw], g[nw:]) for p, g in enumerate(ref["genomes"])
              if p in {int(genome_of[k]) for k in ref["exact"]}}
    worst, worst_shared = 0.0, 0.0
    for a in range(N):
        for i in range(M):
            if (a, i) not in ref["exact"]:
                # dead, unassigned, out of range: neither y nor the action is written
                assert np.array_equal(y[a, i], np.full(4, -7.25)), (a, i, raw[a, i])
                assert after[a, i].tobytes() == before[a, i].tobytes(), (a, i, raw[a, i])
                continue
            p = int(genome_of[a, i])
            worst = max(worst, ec.rel_dev(y[a, i], ref["exact"][a, i]))
            worst_shared = max(worst_shared, ec.rel_dev(y[a, i], shared[p][a, i]))
            d = eo.decode(y[a, i], W, H)                 # the decode of the device's own y, exactly
            got = after[a, i]
            assert [got["valid"], got["shoot"], got["thrust"], got["px"], got["py"], got["_pad"]] == list(d) + [0]
    print("r24 %s: %d ships, worst relative deviation from forward_exact %.3e, from ofx_scratch_feed_obs %.3e"
          % (ec.case_id(case), len(ref["exact"]), worst, worst_shared))
    for (a, i), want in ref["exact"].items():
        np.testing.assert_allclose(y[a, i], want, rtol=rtol, atol=0, err_msg="arena %d ship %d" % (a, i))
        np.testing.assert_allclose(y[a, i], shared[int(genome_of[a, i])][a, i], rtol=rtol, atol=0,
                                   err_msg="arena %d ship %d against ofx_scratch_feed_obs" % (a, i))

    if kind == "dense":
        # a ship's bits do not depend on its company: all 64 ships of arena 0 flown, then ship 0 alone
        assert genome_of[0, 0] == 0 and (0, 0) in ref["exact"]
        crowd = np.full((N, M), -1, np.int32)
        crowd[0] = np.arange(M) % ec.P
        y_crowd, _ = _act(b, pop, crowd)
        alone = np.full((N, M), -1, np.int32)
        alone[0, 0] = 0
        y_alone, _ = _act(b, pop, alone)
        assert np.array_equal(_bits(y_crowd[0, 0]), _bits(y[0, 0])) and np.array_equal(_bits(y_alone[0, 0]), _bits(y[0, 0]))
        assert not (y_crowd[0] == -7.25).any() and (y_alone.reshape(-1, 4)[1:] == -7.25).all()
        # nor on the arena's index: global arena 2 as arena 2 of 3 and as arena 0 of 1
        assert any(a == 2 for a, _ in ref["exact"])
        b1 = ec.case_scene(case).device(1, arena_base=2)
        _assert_scene(b1, ref["obs"][2:])
        pop1 = _population(b1, layers, ref["genomes"])
        y_one, _ = _act(b1, pop1, genome_of[2:3])
        assert np.array_equal(_bits(y_one[0]), _bits(y[2]))
        b1.close()
    b.close()


def test_breed_with_more_jobs_than_grid_rows():
    """70 000 slots of a 273-element genome (153 MB): init is one job per slot and the breed 69 999 jobs, both past the
    65 535 rows of the grid, so k_pop_breed's `j += gridDim.y` loop runs.  n1 = 1: the first layer's transposition is
    the identity."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import Population
    P, layers = 70000, BREED_LAYERS
    assert P * eo.n_elements(layers) * 8 < 200e6
    b = ArenaBatch(1, 1, width=16, height=8)
    pop = Population(b, layers, P, SEED)
    slots = BREED_SLOTS + [P - 2] + [int(p) for p in np.random.RandomState(70).randint(2, P - 2, 32)]
    assert len(BREED_SLOTS) == 7 and BREED_SLOTS[-1] == P - 1
    for p in slots:
        assert np.array_equal(_bits(_flat(pop, p)), _bits(eo.fresh(layers, SEED, p, 0))), "init, slot %d" % p
    plan = np.zeros(P, np.int32)
    plan[P - 2] = -1
    pop.breed(plan, 0.05, 0.05, 1)
    parent = eo.fresh(layers, SEED, 0, 0)
    for p in slots:
        want = parent if p == 0 else eo.fresh(layers, SEED, p, 1) if p == P - 2 else eo.child(parent, SEED, p, 1, 0.05, 0.05)
        assert np.array_equal(_bits(_flat(pop, p)), _bits(want)), "generation 1, slot %d" % p
    b.close()


@pytest.mark.parametrize("n1", [1, 32, 33, 64])
def test_set_then_get_names_every_element(n1):
    """Element e holds the value e: a slip of the first layer's transposition names the element it moved."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.evolution import Population
    W, H, P = 24, 20, 3
    layers = [8 + 2 * W * H, n1, 4]
    b = ArenaBatch(1, 1, width=W, height=H)
    pop = Population(b, layers, P, SEED)
    g = np.arange(eo.n_elements(layers), dtype=np.float64)
    pop.set_genome(1, *eo.split(layers, g))
    got = _flat(pop, 1)
    assert np.array_equal(got, g), "first elements that moved: %s" % np.flatnonzero(got != g)[:8]
    for p in (0, 2):                                       # the neighbours are not touched
        assert np.array_equal(_bits(_flat(pop, p)), _bits(eo.fresh(layers, SEED, p, 0))), "slot %d" % p
    b.close()


def test_fitness_sums_of_either_sign():
    from ofighters_amd import ArenaBatch, _native as nat
    from ofighters_amd.evolution import Population
    N, M, P, W, H = 6, 8, 4, 16, 8
    b = ArenaBatch(N, M, width=W, height=H)
    b.spawn_random(SEED)
    pop = Population(b, [8 + 2 * W * H, 1, 4], P, SEED)
    genome_of = np.full(N * M, -1, np.int32)
    last = np.random.RandomState(6).randint(-1000, 1000, N * M).astype(np.int32)
    genome_of[:40], last[:40] = 2, INT32_MIN               # one genome on 40 ships: -85 899 345 920
    genome_of[40:43], last[40:43] = 0, (-1, INT32_MIN, INT32_MAX)
    genome_of[43:45], last[43:45] = 1, INT32_MAX           # past int32 upwards
    genome_of[45], genome_of[46] = P, INT32_MAX            # out of range: not counted; slot 3 and ship 47 (-1) neither
    last[45:48] = (INT32_MAX, INT32_MIN, -5)

    def put(scores):
        b.sync()
        s = np.ascontiguousarray(scores, np.int32)
        nat.check(nat.lib().ofx_memcpy_h2d(nat.lib().ofx_device_ptr(b.handle, nat.F_LAST_SCORES), _vp(s), s.nbytes))

    def want(scores):
        s, c = np.zeros(P, np.int64), np.zeros(P, np.int32)
        for g in range(P):
            s[g] = scores[genome_of == g].astype(np.int64).sum()
            c[g] = (genome_of == g).sum()
        return s, c

    b.sync()
    pop._genome_of.upload(genome_of)                       # as it is: Population.assign refuses the out-of-range values
    put(last)
    s1, c1 = want(last)
    assert s1[2] == 40 * INT32_MIN and s1[0] == -2 and s1[1] == 2 * INT32_MAX and c1.tolist() == [3, 2, 40, 0]
    pop.fitness(reset=True)
    s, c = pop.fitness_host()
    assert s.dtype == np.int64 and np.array_equal(s, s1) and np.array_equal(c, c1)
    pop.fitness(reset=False)                               # adds
    s, c = pop.fitness_host()
    assert np.array_equal(s, 2 * s1) and np.array_equal(c, 2 * c1)
    other = ~last                                          # -x - 1: every sign flipped, INT32_MIN <-> INT32_MAX
    put(other)
    pop.fitness(reset=False)
    s, c = pop.fitness_host()
    assert np.array_equal(s, 2 * s1 + want(other)[0]) and np.array_equal(c, 3 * c1)
    pop.fitness(reset=True)                                # starts again
    s, c = pop.fitness_host()
    assert np.array_equal(s, want(other)[0]) and np.array_equal(c, c1)
    b.close()


# ---- ofx_scratch_feed / ofx_scratch_feed_obs: the widths and depths tests/test_gpu_obs.py leaves out ----------------
# k_obs_tail works in passes of 8 neurons and a 256-strided final loop: n1 below 8, no multiple of 8, above 256.
ODD, ONE = ("odd", 56, 36, 5, (), 6, 14), ("one", 8, 4, 1, (), 0, 5)     # scenes of ec.FORWARD_CASES; the nets are below
OBS_CASES = [(ODD, [n1, 4]) for n1 in (1, 7, 8, 17, 300)] + \
            [(ODD, [4]), (ODD, [17, 8, 5, 4]), (("dense", 128, 128, 64, (), 0, 5), [9, 4]), (ONE, [9, 4])]


def _oracle_feed(layers, g, obs, M):
    Wl, Bl = eo.split(layers, g)
    return np.stack([np.stack([pyoracle.nn_feed(layers, Wl, Bl, np.concatenate([head[i], sm.ravel(), lm.ravel()]))
                               for i in range(M)]) for head, sm, lm, _ in obs])


@pytest.mark.parametrize("case,tail", OBS_CASES, ids=lambda v: ec.case_id(v) if isinstance(v, tuple) else "x".join(map(str, v)))
def test_scratch_feed_obs_widths_and_depths(case, tail):
    _, W, H, M, _, _, seed = case
    N = 2
    layers = [8 + 2 * W * H] + tail
    sc = ec.case_scene(case)
    obs = [ec.observation(a) for a in sc.oracle(N).arenas]
    b = sc.device(N)
    _assert_scene(b, obs)
    g = ec.scaled_genome(layers, len(ec.set_cells(obs[0][1], obs[0][2])), np.random.RandomState(len(tail) + tail[0]))
    nw = sum(layers[i] * layers[i + 1] for i in range(len(layers) - 1))
    y, am = _feed_obs(b, layers, g[:nw], g[nw:], want_argmax=True)
    want = _oracle_feed(layers, g, obs, M)
    print("r24 scratch_feed_obs %s %s: worst relative deviation from the oracle's feed %.3e" % (ec.case_id(case), tail, ec.rel_dev(y, want)))
    np.testing.assert_allclose(y, want, rtol=1e-12, atol=0)
    assert np.array_equal(am, np.argmax(y, axis=-1))
    b.close()


def _feed(b, layers, W, B, X):
    from ofighters_amd import DeviceBuffer, _native as nat
    larr = np.ascontiguousarray(layers, np.int32)
    w, bb = np.concatenate([a.ravel() for a in W]), np.concatenate([a.ravel() for a in B])
    X = np.ascontiguousarray(X, np.float64)
    assert X.shape[1] == layers[0]
    dw, db, dx = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(bb.nbytes).upload(bb), DeviceBuffer(X.nbytes).upload(X)
    dy, da = DeviceBuffer(8 * len(X) * layers[-1]), DeviceBuffer(4 * len(X))
    nat.check(nat.lib().ofx_scratch_feed(b.handle, _vp(larr), len(layers), dw.ptr, db.ptr, dx.ptr, len(X), dy.ptr, da.ptr))
    b.sync()
    return dy.download(np.float64, (len(X), layers[-1])), da.download(np.int32, (len(X),))


@pytest.mark.parametrize("layers", [[1, 1], [63, 5, 3], [65, 257, 2]], ids=lambda l: "x".join(map(str, l)))
@pytest.mark.parametrize("batch", [1, 33])
def test_scratch_feed_small_and_ragged(layers, batch):
    from ofighters_amd import ArenaBatch
    rs = np.random.RandomState(sum(layers) + batch)
    n = len(layers) - 1
    W = [rs.uniform(-1, 1, (layers[i + 1], layers[i])) / np.sqrt(layers[i]) for i in range(n)]
    B = [rs.uniform(-1, 1, (layers[i + 1], 1)) for i in range(n)]
    X = rs.uniform(-1, 1, (batch, layers[0]))
    b = ArenaBatch(1, 1, width=8, height=4)
    y, am = _feed(b, layers, W, B, X)
    want = np.stack([pyoracle.nn_feed(layers, W, B, x) for x in X])
    np.testing.assert_allclose(y, want, rtol=1e-12, atol=0)
    assert np.array_equal(am, np.argmax(y, axis=1))
    b.close()


def test_scratch_feed_argmax_takes_the_first_of_equal_maxima():
    from ofighters_amd import ArenaBatch
    rs = np.random.RandomState(12)
    layers, batch = [63, 5, 3], 33
    W = [rs.uniform(-1, 1, (5, 63)) / 2, rs.uniform(-1, 1, (3, 5))]
    B = [rs.uniform(-1, 1, (5, 1)), rs.uniform(-1, 1, (3, 1))]
    W[1][2], B[1][2] = W[1][1], B[1][1]                   # outputs 1 and 2 are the same neuron
    W[1][0], B[1][0] = -W[1][1], -B[1][1]                 # and output 0 is 1 - output 1: it wins in some rows
    X = rs.uniform(-1, 1, (batch, 63))
    b = ArenaBatch(1, 1, width=8, height=4)
    y, am = _feed(b, layers, W, B, X)
    assert np.array_equal(_bits(y[:, 1]), _bits(y[:, 2]))
    tied = y[:, 1] > y[:, 0]                              # the oracle's feed: 27 rows against 6, 0.01 apart at the least
    assert tied.sum() >= 5 and (~tied).sum() >= 5
    assert (am[tied] == 1).all() and (am[~tied] == 0).all() and np.array_equal(am, np.argmax(y, axis=1))
    W[1][0], B[1][0] = W[1][1], B[1][1]                   # all three equal: index 0
    y, am = _feed(b, layers, W, B, X)
    assert np.array_equal(_bits(y[:, 0]), _bits(y[:, 2])) and (am == 0).all()
    b.close()


def test_scratch_feed_obs_refuses_a_first_layer_past_its_lds():
    """layers[1] = 2049 would ask for more dynamic LDS than the launch can have: refused up front, nothing enqueued,
    and the handle goes on working."""
    from ofighters_amd import DeviceBuffer, _native as nat
    sc = ec.case_scene(ONE)
    obs = [ec.observation(a) for a in sc.oracle(1).arenas]
    b = sc.device(1)
    wide = np.asarray([72, 2049, 4], np.int32)
    dw, db = DeviceBuffer(8 * (72 * 2049 + 2049 * 4)), DeviceBuffer(8 * (2049 + 4))
    dy = DeviceBuffer(8 * 4)
    rc = nat.lib().ofx_scratch_feed_obs(b.handle, _vp(wide), 3, dw.ptr, db.ptr, dy.ptr, None)
    msg = nat.lib().ofx_last_error().decode()
    assert rc == nat.OFX_ERR_INVALID and "2048" in msg and "2049" in msg and "layers[1]" in msg, (rc, msg)
    layers = [72, 2048 // 64, 4]
    g = ec.scaled_genome(layers, 32, np.random.RandomState(9))
    nw = 72 * 32 + 32 * 4
    y = _feed_obs(b, layers, g[:nw], g[nw:])
    np.testing.assert_allclose(y, _oracle_feed(layers, g, obs, 1), rtol=1e-12, atol=0)
    b.close()
