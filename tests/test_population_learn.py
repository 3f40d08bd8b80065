"""The learning step of the scratch MLP without a GPU: tests/learn_oracle.py (the numpy model of ofx_population_learn's
contract) held to the reference's recorded backprop / update_network, to central differences and to an exactly rounded
twin; the target round trip; EvolutionRollout's imitation hook and state_dict on the oracle stand-in; the checkpoint's
refusals."""
import numpy as np
import pytest

from ofighters_amd import evolution
from tests import evolution_cases as ec
from tests import evolution_oracle as eo
from tests import learn_oracle as lo

TAGS = ("a", "b", "c")


@pytest.fixture(scope="module")
def golden():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scratch_backprop.npz")) as z:
        return {k: z[k] for k in z.files}


def _flat_grad(gw, gb):
    return np.concatenate([w.ravel() for w in gw] + [b.ravel() for b in gb])


@pytest.fixture(scope="module")
def tolerance():
    """(one step, twenty steps): the worst relative difference of an updated weight between the numpy model and its
    exactly rounded twin on the trajectory of lo.TRAJ - the figures the GPU tolerances come from."""
    T, layers, genomes, genome_of, obs, alive, acts = _trajectory_inputs()
    one = twenty = 0.0
    for p in range(T["P"]):
        samples_at = lambda t: _samples(T, genome_of, alive, obs, acts[t], p)
        g_np, g_ex = genomes[p].copy(), genomes[p].copy()
        for t in range(T["steps"]):
            g_np, _, _ = lo.learn(layers, g_np, samples_at(t), T["rate"])
            g_ex = lo.learn_exact(layers, g_ex, samples_at(t), T["rate"])
            if t == 0:
                one = max(one, lo.worst_rel(g_np, g_ex))
        twenty = max(twenty, lo.worst_rel(g_np, g_ex))
    return one, twenty


def _trajectory_inputs():
    T = lo.TRAJ
    layers = [8 + 2 * T["W"] * T["H"]] + list(T["hidden"]) + [4]
    b = ec.scene(T["W"], T["H"], T["M"], T["seed"], T["ticks"]).oracle(T["N"])
    obs, alive = [], []
    for arena in b.arenas:
        head, sm, lm, al = ec.observation(arena)
        obs.append((head, sm, lm))
        alive.append(al)
    genomes = lo.trajectory_genomes(layers, len(ec.set_cells(obs[0][1], obs[0][2])))
    acts = []
    for t in range(T["steps"]):
        b.bot_actions(["random"] * T["M"], T["seed"], tick=T["tick0"] + t)
        acts.append(np.array(b._acts))
    return T, layers, genomes, lo.trajectory_assignment(), obs, np.array(alive), acts


def _samples(T, genome_of, alive, obs, acts, p):
    out = []
    for a in range(T["N"]):
        for i in range(T["M"]):
            sol, valid = lo.targets(acts[a][i], T["W"], T["H"])
            if genome_of[a, i] == p and alive[a, i] and valid:
                out.append((lo.obs_vector(obs[a][0][i], obs[a][1], obs[a][2]), sol))
    return out


# ---------------------------------------------------------------- (a) the reference's recorded numbers
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_equal_the_references_backprop(golden, tag):
    layers = [int(v) for v in golden["layers_" + tag]]
    g = golden["before_" + tag]
    for x, s, want in zip(golden["x_" + tag], golden["sol_" + tag], golden["grad_" + tag]):
        got = _flat_grad(*lo.gradient(layers, g, x, s))
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("n", (1, 2, 5))
def test_updated_weights_equal_update_network(golden, tag, n):
    """rate = 1 on n observations is update_network; the model adds the terms one after the other, the reference sums,
    divides and adds once: equal within the one-step tolerance."""
    layers = [int(v) for v in golden["layers_" + tag]]
    samples = list(zip(golden["x_" + tag][:n], golden["sol_" + tag][:n]))
    new, _, _ = lo.learn(layers, golden["before_" + tag], samples, 1.0)
    want = golden["after%d_%s" % (n, tag)]
    print("update_network %s n=%d: worst relative difference %.3e" % (tag, n, lo.worst_rel(new, want)))
    np.testing.assert_allclose(new, want, rtol=lo.RTOL_STEP, atol=0)
    assert not np.array_equal(new, golden["before_" + tag])


@pytest.mark.parametrize("tag", TAGS)
def test_one_observation_with_a_rate_is_update_network_continuous(golden, tag):
    """update_network_continuous(obs, sol, 0.01) adds 0.01 * gradient.  The reference's own call raises under the numpy
    the fixture was recorded with for layers of different shapes (tools/gen_learn_golden.py says so in cont_ok); its
    formula is then held to the recorded backprop gradient instead."""
    layers = [int(v) for v in golden["layers_" + tag]]
    g, x, s = golden["before_" + tag], golden["x_" + tag][0], golden["sol_" + tag][0]
    new, _, _ = lo.learn(layers, g, [(x, s)], 0.01)
    want = golden["cont_" + tag] if int(golden["cont_ok_" + tag]) else g + 0.01 * golden["grad_" + tag][0]
    np.testing.assert_allclose(new, want, rtol=lo.RTOL_STEP, atol=0)


# ---------------------------------------------------------------- (b) central differences
@pytest.mark.parametrize("tag", TAGS)
def test_gradient_is_minus_the_derivative_of_half_the_squared_error(golden, tag):
    layers = [int(v) for v in golden["layers_" + tag]]
    g, x, s = golden["before_" + tag], golden["x_" + tag][1], golden["sol_" + tag][1]
    got = _flat_grad(*lo.gradient(layers, g, x, s))
    loss = lambda v: 0.5 * float(np.sum((s - lo.activations(layers, v, x)[-1]) ** 2))
    h = 1e-6
    rs = np.random.RandomState(7)
    nz = np.flatnonzero(got)
    for e in np.concatenate([rs.choice(nz, 40, replace=False), np.flatnonzero(got == 0)[:5]]):
        up, dn = g.copy(), g.copy()
        up[e] += h
        dn[e] -= h
        fd = -(loss(up) - loss(dn)) / (2 * h)
        assert abs(fd - got[e]) <= 1e-6 * max(abs(got[e]), 1e-3), "element %d: %.12e against %.12e" % (e, fd, got[e])


# ---------------------------------------------------------------- (c) the targets invert the decode
@pytest.mark.parametrize("W", (48, 80, 400))
def test_targets_round_trip_through_the_decode(W):
    for px in range(W):
        sol, mask = lo.targets((1, 1, 0, px, px % 40), W, 40)
        assert mask and sol[0] == 1.0 and sol[1] == 0.0
        assert int(sol[2] * W) == px and int(sol[3] * 40) == px % 40
        assert 0.0 < sol[2] < 1.0
    for px, want in ((-1, 0.0), (-50, 0.0), (W, 1.0), (W + 7, 1.0)):
        sol, mask = lo.targets((0, 0, 1, px, 3), W, 40)
        assert sol[2] == want and not mask and sol[0] == 0.0 and sol[1] == 1.0


# ---------------------------------------------------------------- (d) the tolerances
def test_model_stays_ten_times_inside_the_gpu_tolerances(tolerance):
    one, twenty = tolerance
    print("numpy model against the exactly rounded twin, worst relative difference of an updated weight: "
          "one step %.3e, twenty steps %.3e" % (one, twenty))
    assert twenty <= lo.MEASURED_20_STEPS, "the recorded twenty-step figure is stale"
    assert one * 10 <= lo.RTOL_STEP
    assert twenty * 10 <= lo.RTOL_TRAJECTORY


def test_imitation_lowers_the_models_error_at_the_trajectorys_rate():
    """The model's summed err against the teacher's twenty actions, before and after the twenty steps at lo.TRAJ's rate."""
    T, layers, genomes, genome_of, obs, alive, acts = _trajectory_inputs()

    def total(gs):
        s = 0.0
        for p in range(T["P"]):
            for t in range(T["steps"]):
                for x, sol in _samples(T, genome_of, alive, obs, acts[t], p):
                    s += lo.err_of(sol - lo.activations(layers, gs[p], x)[-1])
        return s

    after = [g.copy() for g in genomes]
    n = 0
    for t in range(T["steps"]):
        for p in range(T["P"]):
            samples = _samples(T, genome_of, alive, obs, acts[t], p)
            n += len(samples)
            after[p], _, _ = lo.learn(layers, after[p], samples, T["rate"])
    before_err, after_err = total(genomes), total(after)
    print("summed err over %d samples: %.6f before, %.6f after" % (n, before_err, after_err))
    assert n >= 40 and after_err < before_err


# ---------------------------------------------------------------- (e) the loop on the stand-in
class _Batch(eo.EvolutionOracleBatch):
    def state_dict(self):
        return {"episode": self.episode, "lockstep_count": self.lockstep_count}

    def load_state_dict(self, d):
        self.episode, self.lockstep_count = d["episode"], d["lockstep_count"]


def _stand_in(**kw):
    N, M, P, TICKS = 2, 3, 3, 4
    b = _Batch(N, M, 48, 40)
    pop = lo.LearnOraclePopulation(b, [8 + 2 * 48 * 40, 9, 4], P, 77)
    roll = evolution.EvolutionRollout(b, pop, ["random"] * M, 77, ships=(1,), survivors=1, dafts=0, episode_ticks=TICKS,
                                      **kw)
    return b, pop, roll, TICKS


def test_rollout_imitates_for_the_first_generations_then_acts():
    b, pop, roll, T = _stand_in(imitate_rate=0.5, imitate_generations=2)
    start = [g.copy() for g in pop.genomes]
    roll.run(3 * T + 1)
    flights = [c for c in pop.calls if c[0] in ("act", "imitate")]
    assert flights == [("imitate", t) for t in range(2 * T)] + [("act", t) for t in range(2 * T, 3 * T + 1)]
    assert roll.generation == 3 and [e[0] for e in roll.imitation_log] == [0, 1]
    assert all(n > 0 and err > 0 for _, err, n in roll.imitation_log)
    assert any(not np.array_equal(a, c) for a, c in zip(start, pop.genomes))


def test_rollout_defaults_make_todays_calls():
    b, pop, roll, T = _stand_in()
    assert roll.policy == pop.act
    roll.run(2 * T + 1)
    b2 = _Batch(2, 3, 48, 40)
    pop2 = eo.OraclePopulation(b2, [8 + 2 * 48 * 40, 9, 4], 3, 77)
    roll2 = evolution.EvolutionRollout(b2, pop2, ["random"] * 3, 77, ships=(1,), survivors=1, dafts=0, episode_ticks=T)
    roll2.run(2 * T + 1)
    assert len(pop.calls) == len(pop2.calls) and roll.imitation_log == []
    for c1, c2 in zip(pop.calls, pop2.calls):
        assert c1[0] == c2[0] and all(np.array_equal(u, v) for u, v in zip(c1[1:], c2[1:]))
    for rate, gens in ((float("nan"), 1), (-0.1, 1), (0.1, -1)):
        with pytest.raises(ValueError, match="imitate"):
            _stand_in(imitate_rate=rate, imitate_generations=gens)


def test_rollout_state_dict_round_trips():
    b, pop, roll, T = _stand_in(imitate_rate=0.5, imitate_generations=2)
    roll.run(T + 2)                                    # inside the second generation's episode, an imitate call made
    d = roll.state_dict()
    assert d["imitated"] and d["generation"] == 1 and d["tick"] == T + 2 and len(d["plans"]) == 1
    b2, pop2, roll2, _ = _stand_in(imitate_rate=0.5, imitate_generations=2)
    roll2.load_state_dict(d)
    d2 = roll2.state_dict()
    assert sorted(d) == sorted(d2)
    for k in d:
        if k in ("plans", "score_log"):
            assert len(d[k]) == len(d2[k]) and all(np.array_equal(u, v) for u, v in zip(d[k], d2[k]))
        elif isinstance(d[k], np.ndarray):
            assert np.array_equal(d[k], d2[k]), k
        else:
            assert d[k] == d2[k], k
    assert np.array_equal(pop2.genome_of, pop.genome_of)
    with pytest.raises(ValueError, match="'tick'"):
        roll2.load_state_dict({k: v for k, v in d.items() if k != "tick"})


# ---------------------------------------------------------------- (f) the checkpoint's refusals
def test_population_checkpoint_refuses_by_field():
    layers, P, seed = [104, 9, 4], 3, 11
    meta = evolution.population_meta(layers, P, seed)
    shape = (P, sum(evolution.genome_sizes(layers)))
    evolution.check_population_meta(meta, shape, np.float64, layers, P, seed)
    for field, other in (("layers", [104, 8, 4]), ("P", 4), ("seed", 12)):
        with pytest.raises(ValueError, match=field):
            evolution.check_population_meta(dict(meta, **{field: other}), shape, np.float64, layers, P, seed)
        with pytest.raises(ValueError, match=field):
            evolution.check_population_meta({k: v for k, v in meta.items() if k != field}, shape, np.float64, layers, P, seed)
    with pytest.raises(ValueError, match="shape"):
        evolution.check_population_meta(meta, (P, shape[1] - 1), np.float64, layers, P, seed)
    with pytest.raises(ValueError, match="dtype"):
        evolution.check_population_meta(meta, shape, np.float32, layers, P, seed)
    assert evolution.sidecar_path("pop.npy") == "pop.npy.json"
