"""Neuroevolution of the scratch MLP, the CPU side: the oracle's own properties, truncation_plan, the refusals of the
Python layer, the entry points in header / binding / library, and EvolutionRollout's host logic on an oracle-backed
stand-in (the population held by the oracle).  The kernels are held to the same oracle in tests/test_gpu_evolution.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from ofighters_amd import _native as nat
from ofighters_amd import evolution
from tests import evolution_oracle as eo
from tests.abi_header import header_symbols

LAYERS = [8 + 2 * 48 * 40, 9, 4]
SEED = 0x0E701234


def test_entry_points_declared_bound_and_exported():
    declared, L = header_symbols(), C.CDLL(nat.LIB_PATH)
    for s in ("ofx_population_create", "ofx_population_destroy", "ofx_population_init", "ofx_population_get",
              "ofx_population_set", "ofx_population_breed", "ofx_population_act", "ofx_population_fitness"):
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    assert nat.SIGNATURES["ofx_population_create"][1][3] is C.c_int64       # P is 64-bit
    assert nat.SIGNATURES["ofx_population_breed"][1][2:] == [C.c_double, C.c_double, C.c_uint64, C.c_uint32]


def test_uniform_is_numpys_53_bit_double():
    assert eo.u(0, 0) == 0.0
    top = eo.u(0xFFFFFFFF, 0xFFFFFFFF)
    assert top < 1.0 and top == 1.0 - 2.0 ** -53
    assert eo.u(1 << 5, 0) == 2.0 ** -27 and eo.u(0, 1 << 6) == 2.0 ** -53 and eo.u(31, 63) == 0.0
    # arrays draw the words pyoracle.philox draws
    r = pyoracle.philox(3, 77, 2, eo.STREAM_FRESH, SEED)
    assert eo.fresh(LAYERS, SEED, 3, 2, elements=[77])[0] == 2.0 * float(eo.u(r[0], r[1])) - 1.0 == eo.fresh_scalar(SEED, 3, 77, 2)


def test_oracle_init_and_breed_properties():
    P = 5
    pop = [eo.fresh(LAYERS, SEED, p, 0) for p in range(P)]
    for g in pop:
        assert g.shape == (eo.n_elements(LAYERS),) and (g >= -1.0).all() and (g < 1.0).all()
    assert not np.array_equal(pop[0], pop[1])
    plan = np.array([0, 0, -1, 3, 3], np.int32)
    # a kept slot is unchanged; rates (0, 0) give an exact copy of the parent
    out = eo.breed(pop, plan, 0.0, 0.0, SEED, 1, LAYERS)
    assert out[0] is pop[0] and out[3] is pop[3]
    assert np.array_equal(out[1], pop[0]) and np.array_equal(out[4], pop[3])
    assert np.array_equal(out[2], eo.fresh(LAYERS, SEED, 2, 1)) and not np.array_equal(out[2], pop[2])
    # mutated elements are exactly those with u_sel < rate, and they lie in [-1, 1)
    out = eo.breed(pop, plan, 0.0, 0.3, SEED, 1, LAYERS)
    sel = eo.selector(LAYERS, SEED, 1, 1) < 0.3
    assert 0.25 < sel.mean() < 0.35
    assert np.array_equal(out[1][~sel], pop[0][~sel]) and (out[1][sel] != pop[0][sel]).all()
    assert (out[1][sel] >= -1.0).all() and (out[1][sel] < 1.0).all()
    # evolution alone: |w' - w| <= rate |w| up to the three roundings (each below 2^-52 |w|, i.e. 1e-15 of rate |w|),
    # and every element moves by its own coefficient
    out = eo.breed(pop, plan, 0.3, 0.0, SEED, 1, LAYERS)
    assert (np.abs(out[1] - pop[0]) <= 0.3 * np.abs(pop[0]) * (1 + 1e-14)).all()
    assert (out[1] != pop[0]).mean() > 0.99
    # another generation, another slot: other draws
    assert not np.array_equal(eo.child(pop[0], SEED, 1, 1, 0.05, 0.05), eo.child(pop[0], SEED, 1, 2, 0.05, 0.05))
    assert not np.array_equal(eo.child(pop[0], SEED, 1, 1, 0.05, 0.05), eo.child(pop[0], SEED, 2, 1, 0.05, 0.05))


def test_oracle_forward_is_the_dense_feed():
    """The sparse first layer of the oracle == pyoracle.nn_feed on the materialised toVector()."""
    rs = np.random.RandomState(5)
    arena = pyoracle.Arena(cfg=pyoracle.default_cfg(3, width=48, height=40))
    arena.spawn(np.array([[10, 12], [30, 20], [40, 33]], np.int32))
    sm, lm = arena.rasterise()
    head, _ = arena.obs_head()
    for layers in (LAYERS, [LAYERS[0], 13, 7, 4]):
        g = rs.uniform(-1, 1, eo.n_elements(layers))
        W, B = eo.split(layers, g)
        for i in range(3):
            vec = np.concatenate([head[i], sm.ravel(), lm.ravel()]).astype(np.float64)
            want = pyoracle.nn_feed(layers, W, B, vec)
            np.testing.assert_allclose(eo.forward(layers, g, head[i], sm, lm), want, rtol=1e-12, atol=0)
    assert list(eo.decode(np.array([0.6, 0.5, 0.999, 0.0]), 48, 40)) == [1, 1, 0, 47, 0]


def test_genome_split_and_join_round_trip():
    layers = [20, 5, 4]
    nw, nb = evolution.genome_sizes(layers)
    assert (nw, nb) == (120, 9)
    w, b = np.arange(nw, dtype=np.float64), np.arange(nb, dtype=np.float64) + 1000
    W, B = evolution.split_genome(layers, w, b)
    assert [a.shape for a in W] == [(5, 20), (4, 5)] and [a.shape for a in B] == [(5, 1), (4, 1)]
    w2, b2 = evolution.join_genome(layers, W, B)
    assert np.array_equal(w, w2) and np.array_equal(b, b2)
    Wo, Bo = eo.split(layers, np.concatenate([w, b]))
    assert all(np.array_equal(x, y) for x, y in zip(W + B, Wo + Bo))
    with pytest.raises(ValueError):
        evolution.join_genome(layers, W[::-1], B)


def test_truncation_plan():
    tp = evolution.truncation_plan
    # ranks: slot 3 (mean 9), then 0 and 2 tied at 5 (the lower slot first), 4 (mean 1), 1 (never flown)
    s, c = np.array([10, 0, 5, 9, 2], np.int64), np.array([2, 0, 1, 1, 2], np.int32)
    assert list(tp(s, c, 2, 1)) == [0, -1, 3, 3, 0]
    assert list(tp(s, c, 1, 0)) == [3, 3, 3, 3, 3]
    assert list(tp(s, c, 5, 0)) == [0, 1, 2, 3, 4]            # survivors = P: nothing changes
    assert list(tp(s, c, 2, 3)) == [0, -1, -1, 3, -1]
    assert list(tp(s, c, 3, 0)) == [0, 0, 2, 3, 3]            # children dealt round-robin: rank 4 -> 3, rank 5 -> 0
    # all tied: the lowest slots survive
    assert list(tp(np.zeros(4, np.int64), np.ones(4, np.int32), 2, 0)) == [0, 1, 0, 1]
    # negative scores rank above slots nobody flew
    assert list(tp(np.array([-5, 0], np.int64), np.array([1, 0], np.int32), 1, 0)) == [0, 0]
    rs = np.random.RandomState(0)
    for _ in range(50):
        P = int(rs.randint(1, 12))
        surv = int(rs.randint(1, P + 1))
        dafts = int(rs.randint(0, P - surv + 1))
        s, c = rs.randint(-20, 20, P).astype(np.int64), rs.randint(0, 3, P).astype(np.int32)
        plan = tp(s, c, surv, dafts)
        assert plan.dtype == np.int32
        evolution.check_plan(plan, P)
        eo.check_plan(plan, P)
        assert (plan == np.arange(P)).sum() == surv and (plan == -1).sum() == dafts
        assert np.array_equal(plan, tp(s, c, surv, dafts))
    for bad in ((0, 0), (6, 0), (2, 4), (2, -1)):
        with pytest.raises(ValueError):
            tp(np.zeros(5, np.int64), np.ones(5, np.int32), *bad)


def test_python_layer_refuses_bad_plans_and_assignments():
    evolution.check_plan([0, 0, -1, 3], 4)
    with pytest.raises(ValueError, match="not kept"):
        evolution.check_plan([1, 2, 2, 3], 4)                # slot 0's parent 1 is itself a child
    with pytest.raises(ValueError, match="not kept"):
        evolution.check_plan([0, 2, -1, 3], 4)               # slot 1's parent 2 is refreshed
    for bad in ([0, 1, 2, 4], [0, 1, 2, -2]):
        with pytest.raises(ValueError, match="outside"):
            evolution.check_plan(bad, 4)
    with pytest.raises(ValueError):
        evolution.check_plan([0, 1, 2], 4)
    with pytest.raises(ValueError):
        evolution.check_plan(np.zeros(4), 4)                 # floats
    ok = np.full((3, 2), -1, np.int64)
    ok[1, 1] = 3
    assert evolution.check_assignment(ok, 3, 2, 4).dtype == np.int32
    for v in (4, -2):                                        # P and -2
        bad = ok.copy()
        bad[2, 0] = v
        with pytest.raises(ValueError, match="outside"):
            evolution.check_assignment(bad, 3, 2, 4)
    with pytest.raises(ValueError):
        evolution.check_assignment(ok, 2, 3, 4)


N, M, P, TICKS = 3, 3, 4, 6


def _run(ships=(0, 2), base=0):
    b = eo.EvolutionOracleBatch(N, M, 48, 40, arena_base=base)
    pop = eo.OraclePopulation(b, LAYERS, P, SEED)
    roll = evolution.EvolutionRollout(b, pop, ["random"] * M, SEED, ships=ships, survivors=2, dafts=1,
                                      episode_ticks=TICKS)
    roll.run(3 * TICKS + 1)                                  # the third generation ends at the head of lock-step 18
    return b, pop, roll


@pytest.fixture(scope="module")
def stand_in_run():
    return _run()


def test_evolution_rollout_on_the_stand_in(stand_in_run):
    b, pop, roll = stand_in_run
    assert roll.observe is False and roll.generation == 3 and len(roll.fitness_log) == 3 and len(roll.score_log) == 3
    kinds = [c[0] for c in pop.calls]
    # act on every lock-step, once, before the step
    acts = [c[1] for c in pop.calls if c[0] == "act"]
    assert acts == list(range(3 * TICKS + 1))
    # fitness at every episode end (reset: one episode per generation), one breed per generation with generation + 1
    assert [c for c in pop.calls if c[0] == "fitness"] == [("fitness", True)] * 3
    assert [c[1] for c in pop.calls if c[0] == "breed"] == [1, 2, 3]
    # the order at an episode end: ... act(5) | fitness, breed, assign | act(6) ...
    i = kinds.index("fitness")
    assert kinds[i:i + 4] == ["fitness", "breed", "assign", "act"] and pop.calls[i - 1] == ("act", TICKS - 1)
    # genome_of by the formula, re-assigned after every breed
    assigns = [c[1] for c in pop.calls if c[0] == "assign"]
    assert len(assigns) == 4
    for gen, got in enumerate(assigns):
        want = np.full((N, M), -1, np.int32)
        for a in range(N):
            for k, ship in enumerate((0, 2)):
                want[a, ship] = ((0 + a) * 2 + k + gen) % P
        assert np.array_equal(got, want) and np.array_equal(got, roll.assignment(gen))
    # the plans bred on are valid and are truncation_plan's
    for plan in roll.plans:
        eo.check_plan(plan, P)
        assert (plan == np.arange(P)).sum() == 2 and (plan == -1).sum() == 1
    for best, mean in roll.fitness_log:
        assert best >= mean


def test_evolution_rollout_is_reproducible_and_keyed_by_global_arena(stand_in_run):
    _, pop, roll = stand_in_run
    _, pop2, roll2 = _run()
    assert roll.fitness_log == roll2.fitness_log
    assert all(np.array_equal(x, y) for x, y in zip(pop.genomes, pop2.genomes))
    assert all(np.array_equal(x, y) for x, y in zip(roll.plans, roll2.plans))
    b3, pop3, roll3 = _run(base=5)
    assert roll3.assignment(1)[1, 2] == ((5 + 1) * 2 + 1 + 1) % P


def test_evolution_rollout_evolved_ships_fly_the_decoded_output():
    """A lock-step of the stand-in: the evolved ships' actions are the oracle forward's decode, the others the bots'."""
    b = eo.EvolutionOracleBatch(N, M, 48, 40)
    pop = eo.OraclePopulation(b, LAYERS, P, SEED)
    roll = evolution.EvolutionRollout(b, pop, ["random"] * M, SEED, ships=(1,), survivors=1, dafts=0, episode_ticks=TICKS)
    bots = [a.bot_actions(np.full(M, nat.BOT_RANDOM, np.int32), SEED, g, 0) for g, a in enumerate(b.arenas)]
    want = []
    for g, a in enumerate(b.arenas):
        sm, lm = a.rasterise()
        head, _ = a.obs_head()
        want.append(eo.decode(eo.forward(LAYERS, pop.genomes[roll.assignment(0)[g, 1]], head[1], sm, lm), 48, 40))
    b.bot_actions(roll.behaviours, SEED, tick=0)
    pop.act(b)
    for g in range(N):
        assert np.array_equal(b._acts[g][1], want[g]) and want[g][0] == 1
        assert np.array_equal(b._acts[g][[0, 2]], bots[g][[0, 2]])


def test_evolution_rollout_refuses():
    b = eo.EvolutionOracleBatch(1, 2, 48, 40)
    pop = eo.OraclePopulation(b, LAYERS, 2, SEED)
    kw = dict(survivors=1, dafts=0)
    with pytest.raises(ValueError, match="dist"):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, dist=object(), **kw)
    with pytest.raises(ValueError):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, ships=(2,), **kw)
    with pytest.raises(ValueError):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, ships=(0, 0), **kw)
    with pytest.raises(ValueError):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, survivors=3, dafts=0)
    with pytest.raises(ValueError):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, episodes_per_generation=0, **kw)
    with pytest.raises(ValueError):
        evolution.EvolutionRollout(b, pop, ["random"] * 2, SEED, observe=True, **kw)
