"""Seeded evolution strategies on the GPU: members, the forward against the stored-genome forward, the generation step,
fitness and the loop, each against tests/es_oracle.py (numpy float64, the contract of include/ofx.h).  Every comparison
is == on bits unless it says otherwise."""
import numpy as np
import pytest

from tests import es_oracle as so
from tests import evolution_oracle as eo
from tests.es_cases import SEED, bits as _bits, vp as _vp

pytestmark = pytest.mark.gpu


def _centre(es):
    """The centre of an ES as one element vector, through ofx_es_get."""
    return np.concatenate(es.b.es_get(es.n_weights, es.n_biases))


def _member(es, m, P, sigma, generation):
    return np.concatenate(es.b.es_member(m, P, sigma, es.seed, generation, es.n_weights, es.n_biases))


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


# ---------------------------------------------------------------- 1. members
@pytest.mark.parametrize("hidden", [(9,), (13, 7)])
@pytest.mark.parametrize("source", ["init", "set"])
def test_members_bit_for_bit(hidden, source):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    W, H, P, sigma, generation = 48, 40, 6, 0.07, 3
    layers = [8 + 2 * W * H] + list(hidden) + [4]
    b = ArenaBatch(1, 1, width=W, height=H)
    es = ES(b, layers, SEED)
    theta = eo.fresh(layers, SEED, 0, 0)
    if source == "set":
        theta = np.random.RandomState(8).uniform(-1, 1, eo.n_elements(layers))
        theta[:3] = [-0.0, 5e-324, 1.0]
        theta[-1] = -0.0
        es.set_centre(*eo.split(layers, theta))
    assert np.array_equal(_bits(_centre(es)), _bits(theta)), "the centre"
    e = np.arange(theta.size, dtype=np.int64)
    for m in range(P + 1):
        got = _member(es, m, P, sigma, generation)
        assert np.array_equal(_bits(got), _bits(so.member(theta, SEED, m, P, sigma, generation))), "member %d" % m
    assert np.array_equal(_bits(_member(es, P, P, sigma, generation)), _bits(theta)), "member P is the centre"
    for i in range(P // 2):
        noise = so.eps(SEED, i, e, generation)
        plus, minus = np.multiply(sigma, noise), np.multiply(-sigma, noise)
        assert np.array_equal(_bits(plus), _bits(-minus)) and plus.any()
        assert np.array_equal(_bits(_member(es, 2 * i, P, sigma, generation)), _bits(theta + plus))
        assert np.array_equal(_bits(_member(es, 2 * i + 1, P, sigma, generation)), _bits(theta + minus))
    # another generation: other members; the Python layer returns the same bits in the reference's shapes
    assert not np.array_equal(_member(es, 0, P, sigma, generation + 1), _member(es, 0, P, sigma, generation))
    Wl, Bl = es.member(2, P, sigma, generation)
    Wo, Bo = eo.split(layers, so.member(theta, SEED, 2, P, sigma, generation))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(Wl + Bl, Wo + Bo))
    assert np.array_equal(_bits(_centre(es)), _bits(theta)), "materialising members changed the centre"
    b.close()


# ---------------------------------------------------------------- 2. the forward equals the stored-genome forward
def _assignment(N, M, P):
    """A -1; the centre (P); both signs of pair 0 (members 0 and 1); member 1 on two ships of arena 0; (N-1, 1) is the
    ship that gets killed.  Ships behind the third (M = 13: a crowded arena, where the scene's lasers destroy some) go
    through -1, 0, .., P in turn."""
    g = np.full((N, M), -1, np.int32)
    for a in range(N):
        for i in range(3, M):
            g[a, i] = (5 * a + i) % (P + 2) - 1
    g[0, 0], g[0, 1], g[0, 2] = 1, 1, 0
    g[N - 1, 0], g[N - 1, 1] = P, 0
    if N > 2:
        g[1, 0], g[1, 1], g[1, 2] = P, 2 % P, 3 % P
    return g


FORWARD_CASES = [(48, 40, M, hidden) for M in (3, 13) for hidden in ((9,), (13, 7))] + \
                [(80, 52, M, hidden) for M in (3, 13) for hidden in ((9,), (13, 7))] + [(400, 400, 3, (9,))]


@pytest.mark.parametrize("W,H,M,hidden", FORWARD_CASES)
def test_forward_equals_the_stored_genome_forward(W, H, M, hidden):
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.es import ES
    from ofighters_amd.evolution import Population
    big = W == 400
    N, P = (2, 2) if big else (3, 4)
    sigma, generation = 0.02, 5
    layers = [8 + 2 * W * H] + list(hidden) + [4]
    b = ArenaBatch(N, M, width=W, height=H)
    _scene(b, SEED)
    es = ES(b, layers, SEED)
    pop = Population(b, layers, P + 1, SEED)                 # on the same handle: slot m holds member m, slot P the centre
    es.set_centre(*_scaled_genome(layers, np.random.RandomState(3)))
    theta = _centre(es)
    member_of = _assignment(N, M, P)
    assert (member_of == -1).any() and (member_of == P).any() and (member_of == 0).any() and (member_of[0, :2] == 1).all()
    es.assign(member_of, P)
    pop.assign(member_of)
    alive = b.get(nat.F_SHIP_ALIVE)
    flown = (member_of >= 0) & (alive != 0)
    assert not flown[N - 1, 1] and member_of[N - 1, 1] >= 0 and flown.sum() >= 3
    assert {0, 1, P} <= set(int(v) for v in member_of[flown]), "both signs of pair 0 and the centre fly"
    want_member = {}
    for m in (int(v) for v in np.unique(member_of[flown])):
        got = _member(es, m, P, sigma, generation)
        want_member[m] = so.member(theta, SEED, m, P, sigma, generation)
        assert np.array_equal(_bits(got), _bits(want_member[m])), "member %d" % m
        pop.set_genome(m, *eo.split(layers, got))

    sentinel = np.full((N, M, 4), -7.25)
    dy_pop, dy_es = DeviceBuffer(sentinel.nbytes).upload(sentinel), DeviceBuffer(sentinel.nbytes).upload(sentinel)
    b.bot_actions(["random"] * M, SEED, tick=100)
    before = b.actions_host()
    pop.act(y_ptr=dy_pop.ptr)
    b.sync()
    y_pop, act_pop = dy_pop.download(np.float64, (N, M, 4)), b.actions_host()
    b.bot_actions(["random"] * M, SEED, tick=100)            # the bots' actions again: the same bytes
    assert b.actions_host().tobytes() == before.tobytes()
    es.act(sigma, generation, y_ptr=dy_es.ptr)
    b.sync()
    y, act_es = dy_es.download(np.float64, (N, M, 4)), b.actions_host()
    es.act(sigma, generation, y_ptr=dy_es.ptr)
    b.sync()
    assert np.array_equal(_bits(y), _bits(dy_es.download(np.float64, (N, M, 4)))), "a second call gives other bits"
    assert act_es.tobytes() == b.actions_host().tobytes()

    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_F64)
    for a in range(N):
        for i in range(M):
            if not flown[a, i]:
                # dead, unassigned: neither y nor the action is written
                assert np.array_equal(y[a, i], sentinel[a, i])
                assert act_es[a, i].tobytes() == before[a, i].tobytes()
                continue
            m = int(member_of[a, i])
            assert np.array_equal(_bits(y[a, i]), _bits(y_pop[a, i])), "arena %d ship %d member %d: y" % (a, i, m)
            assert act_es[a, i].tobytes() == act_pop[a, i].tobytes(), "arena %d ship %d member %d: action" % (a, i, m)
            want = eo.forward(layers, want_member[m], head[a, i], sm[a], lm[a])
            print("case %dx%d M=%d %s arena %d ship %d member %d: max rel err against numpy %.3e"
                  % (W, H, M, hidden, a, i, m, np.max(np.abs(y[a, i] - want) / np.abs(want))))
            np.testing.assert_allclose(y[a, i], want, rtol=1e-12, atol=0)
            d = eo.decode(y[a, i], W, H)                     # the decode of the device's own y, exactly
            got = act_es[a, i]
            assert [got["valid"], got["shoot"], got["thrust"], got["px"], got["py"], got["_pad"]] == list(d) + [0]
    assert np.array_equal(_bits(_centre(es)), _bits(theta)), "acting changed the centre"
    b.close()


# ---------------------------------------------------------------- 3. the generation step
def test_update_bit_for_bit():
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    W, H = 48, 40
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(1, 1, width=W, height=H)
    es = ES(b, layers, SEED)
    theta = eo.fresh(layers, SEED, 0, 0)
    d = np.array([0.4, 0.0, -1.0])
    for generation, scale in ((0, 0.75), (1, -0.031)):
        b.es_update(d, scale, SEED, generation)
        theta = so.update(theta, d, scale, SEED, generation)
        assert np.array_equal(_bits(_centre(es)), _bits(theta)), "generation %d" % generation
    # through the Python layer: scale = lr / (n_c * sigma), computed in that order
    es.update(d, 0.1, 0.05, 6, 2)
    theta = so.update(theta, d, 0.1 / (6 * 0.05), SEED, 2)
    assert np.array_equal(_bits(_centre(es)), _bits(theta))
    # all weights zero: theta + scale * 0.0
    b.es_update(np.zeros(3), 0.5, SEED, 3)
    assert np.array_equal(_bits(_centre(es)), _bits(so.update(theta, np.zeros(3), 0.5, SEED, 3)))
    b.close()


def test_update_at_the_reference_size():
    """[320008, 9, 4], 2 pairs: a fixed sample of elements that crosses the input-major / element-order mapping at full
    size - the first 4096, the last 4096 (second layer and biases), every 997th in between."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    layers = [320008, 9, 4]
    G = eo.n_elements(layers)
    assert G == 2880121
    sample = np.unique(np.concatenate([np.arange(4096), np.arange(4096, G - 4096, 997), np.arange(G - 4096, G)]))
    b = ArenaBatch(1, 1)
    es = ES(b, layers, SEED)
    theta = eo.fresh(layers, SEED, 0, 0, elements=sample)
    assert np.array_equal(_bits(_centre(es)[sample]), _bits(theta))
    d, scale, generation = np.array([0.6, -0.25]), 1.5, 7
    b.es_update(d, scale, SEED, generation)
    want = so.update(theta, d, scale, SEED, generation, elements=sample)
    got = _centre(es)
    assert np.array_equal(_bits(got[sample]), _bits(want))
    assert (got[sample] != theta).mean() > 0.99
    # a member at this size, on the same sample
    m = _member(es, 3, 4, 0.05, generation)
    assert np.array_equal(_bits(m[sample]), _bits(so.member(want, SEED, 3, 4, 0.05, generation, elements=sample)))
    b.close()


# ---------------------------------------------------------------- 4. fitness and the loop
def test_fitness_sums_with_the_centre_slot():
    from ofighters_amd import ArenaBatch, _native as nat
    from ofighters_amd.es import ES
    N, M, P, W, H = 5, 4, 6, 48, 40
    b = ArenaBatch(N, M, width=W, height=H)
    b.spawn_random(SEED)
    es = ES(b, [8 + 2 * W * H, 9, 4], SEED)
    rs = np.random.RandomState(2)
    member_of = rs.randint(-1, P - 1, (N, M)).astype(np.int32)      # member P - 1 is flown by nobody
    member_of[N - 1, :2] = P                                        # two ships of the last arena fly the centre
    es.assign(member_of, P)
    want_s, want_c = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int32)
    tick = 0
    for episode in range(3):
        for _ in range(12):
            b.bot_actions(["shoot", "random", "turret", "random"], SEED, tick=tick)
            es.act(0.05, episode)
            b.step()
            tick += 1
        b.restart_random(SEED)
        es.fitness(reset=episode == 1)                   # the second episode starts the sums again, the third adds
        last = b.get(nat.F_LAST_SCORES)
        if episode == 1:
            want_s[:], want_c[:] = 0, 0
        for m in range(P + 1):
            want_s[m] += int(last[member_of == m].sum())
            want_c[m] += int((member_of == m).sum())
        s, c = es.fitness_host()
        assert s.dtype == np.int64 and c.dtype == np.int32 and s.shape == c.shape == (P + 1,)
        assert np.array_equal(s, want_s) and np.array_equal(c, want_c), "episode %d" % episode
    assert want_s.any() and want_c[P - 1] == 0 and want_c[P] == 4
    b.close()


LOOP = dict(N=8, M=3, P=4, W=48, H=40, T=10, sigma=0.05, lr=0.2, eval_arenas=2)


def _rollout(seed):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES, ESRollout
    L = LOOP
    layers = [8 + 2 * L["W"] * L["H"], 9, 4]
    b = ArenaBatch(L["N"], L["M"], width=L["W"], height=L["H"])
    es = ES(b, layers, seed)
    roll = ESRollout(b, es, ["random"] * L["M"], seed, L["P"], L["sigma"], L["lr"], ships=(0,),
                     eval_arenas=L["eval_arenas"], episode_ticks=L["T"])
    return b, es, roll


def _loop(seed):
    b, es, roll = _rollout(seed)
    T = LOOP["T"]
    snaps = [_centre(es)]
    for _ in range(3):
        roll.run(T + (1 if len(snaps) == 1 else 0))      # up to and including the lock-step that ends a generation
        snaps.append(_centre(es))
    out = dict(fitness_log=list(roll.fitness_log), centre_log=list(roll.centre_log), weight_log=list(roll.weight_log),
               snaps=snaps, generation=roll.generation, assignment=es.member_of.copy(), want_assignment=roll.assignment(3),
               tick=roll.tick)
    b.close()
    return out


@pytest.fixture(scope="module")
def loop_run():
    return _loop(SEED)


def test_es_loop_on_the_device(loop_run):
    r1, r2 = loop_run, _loop(SEED)
    L = LOOP
    assert r1["generation"] == 3 and len(r1["fitness_log"]) == len(r1["centre_log"]) == len(r1["weight_log"]) == 3
    assert r1["fitness_log"] == r2["fitness_log"] and r1["centre_log"] == r2["centre_log"]
    for s1, s2 in zip(r1["snaps"], r2["snaps"]):
        assert np.array_equal(_bits(s1), _bits(s2))
    assert np.array_equal(r1["assignment"], r1["want_assignment"])
    assert (r1["assignment"][L["N"] - L["eval_arenas"]:, 0] == L["P"]).all()
    # every generation's centre is the oracle's update of the previous one with the recorded weights
    moved = 0
    for gen, (d, n_c) in enumerate(r1["weight_log"]):
        old, new = r1["snaps"][gen], r1["snaps"][gen + 1]
        assert d.shape == (L["P"] // 2,)
        if n_c < 2:
            assert np.array_equal(_bits(old), _bits(new))
            continue
        want = so.update(old, d, L["lr"] / (n_c * L["sigma"]), SEED, gen)
        assert np.array_equal(_bits(new), _bits(want)), "generation %d" % gen
        moved += int(d.any())
    print("weights per generation:", [(list(d), n) for d, n in r1["weight_log"]], "centre_log:", r1["centre_log"])
    assert all(n_c == L["P"] for _, n_c in r1["weight_log"]), "six learning arenas fly all four members"
    assert moved >= 1, "no generation of this seed had an untied pair: the comparison above saw no update"


def test_es_loop_resumes_bit_for_bit(loop_run, tmp_path):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES, ESRollout
    L, T = LOOP, LOOP["T"]
    b, es, roll = _rollout(SEED)
    roll.run(T + 4)                                      # inside the second generation's episode
    path = es.save(str(tmp_path / "centre.npy"))
    state = roll.state_dict()
    assert state["generation"] == 1 and np.array_equal(_bits(_centre(es)), _bits(loop_run["snaps"][1]))
    b.close()
    b2, es2, roll2 = _rollout(SEED + 1)                  # fresh handles; another seed would be refused by load
    with pytest.raises(ValueError, match="seed"):
        es2.load(path)
    b2.close()
    layers = [8 + 2 * L["W"] * L["H"], 9, 4]
    b3 = ArenaBatch(L["N"], L["M"], width=L["W"], height=L["H"])
    es3 = ES(b3, layers, SEED, init=False)
    es3.load(path)
    roll3 = ESRollout(b3, es3, ["random"] * L["M"], SEED, L["P"], L["sigma"], L["lr"], ships=(0,),
                      eval_arenas=L["eval_arenas"], episode_ticks=T)
    roll3.load_state_dict(state)
    roll3.run(loop_run["tick"] - (T + 4))
    assert roll3.generation == 3 and roll3.tick == loop_run["tick"]
    assert roll3.fitness_log == loop_run["fitness_log"] and roll3.centre_log == loop_run["centre_log"]
    assert np.array_equal(_bits(_centre(es3)), _bits(loop_run["snaps"][3]))
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(roll3.weight_log, loop_run["weight_log"]))
    b3.close()


# ---------------------------------------------------------------- 5. refusals and coexistence
def test_refusals_leave_the_centre_unchanged():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    W, H = 48, 40
    nin = 8 + 2 * W * H
    layers = [nin, 9, 4]
    L = nat.lib()
    b = ArenaBatch(2, 2, width=W, height=H)
    h = b.handle
    nw, nb = nin * 9 + 36, 13
    w, bias = np.zeros(nw), np.zeros(nb)
    member_of = DeviceBuffer(16).upload(np.array([[0, 1], [2, -1]], np.int32))
    acts, s8, c4 = DeviceBuffer(12 * 4), DeviceBuffer(8 * 5), DeviceBuffer(4 * 5)
    d = np.array([0.5, -0.5])

    def calls(P=4, sigma=0.05):
        return {"init": lambda: L.ofx_es_init(h, SEED, 0),
                "get": lambda: L.ofx_es_get(h, _vp(w), _vp(bias)),
                "set": lambda: L.ofx_es_set(h, _vp(w), _vp(bias)),
                "member": lambda: L.ofx_es_member(h, 1, P, sigma, SEED, 0, _vp(w), _vp(bias)),
                "act": lambda: L.ofx_es_act(h, member_of.ptr, P, sigma, SEED, 0, acts.ptr, None),
                "fitness": lambda: L.ofx_es_fitness(h, member_of.ptr, P, s8.ptr, c4.ptr, 1),
                "update": lambda: L.ofx_es_update(h, _vp(d), 2, 0.1, SEED, 0)}

    # no centre: every call but create is refused with OFX_ERR_STATE
    for name, call in calls().items():
        assert call() == nat.OFX_ERR_STATE and b"no ES centre" in L.ofx_last_error(), name
    # the refusals of ofx_population_create, minus P
    for bad, word in (([nin + 1, 9, 4], "8 + 2*W*H"), ([nin, 9, 3], "4 outputs"), ([nin, 65, 4], "wide"),
                      ([nin] + [5] * 7 + [4], "layers")):
        with pytest.raises(OfxError) as e:
            b.es_create(bad)
        assert e.value.code == nat.OFX_ERR_INVALID and word in str(e.value) and "ofx_es_create" in str(e.value)
    assert L.ofx_es_create(h, None, 3) == nat.OFX_ERR_INVALID
    b.es_create(layers)
    with pytest.raises(OfxError, match="already") as e:
        b.es_create(layers)
    assert e.value.code == nat.OFX_ERR_STATE
    b.es_init(SEED, 0)
    b.spawn_random(SEED)
    theta = np.concatenate(b.es_get(nw, nb))
    assert np.array_equal(_bits(theta), _bits(eo.fresh(layers, SEED, 0, 0)))

    refused = []
    for P in (3, 1, 0, -2):                                  # P odd or < 2
        for name in ("member", "act", "fitness"):
            refused.append(("P = %d, %s" % (P, name), calls(P=P)[name], b"P must"))
    for sigma in (0.0, -0.05, float("nan"), float("inf")):   # sigma not finite or <= 0
        for name in ("member", "act"):
            refused.append(("sigma = %r, %s" % (sigma, name), calls(sigma=sigma)[name], b"sigma"))
    for scale in (float("nan"), float("inf"), float("-inf")):
        refused.append(("scale = %r" % scale, lambda scale=scale: L.ofx_es_update(h, _vp(d), 2, scale, SEED, 0), b"scale"))
    for v in (float("nan"), float("inf")):
        bad_d = np.array([0.5, v])
        refused.append(("d[1] = %r" % v, lambda bad_d=bad_d: L.ofx_es_update(h, _vp(bad_d), 2, 0.1, SEED, 0), b"d[1]"))
    refused.append(("n_pairs = 0", lambda: L.ofx_es_update(h, _vp(d), 0, 0.1, SEED, 0), b"n_pairs"))
    for m in (-1, 5):                                        # member outside [0, P]
        refused.append(("member %d" % m, lambda m=m: L.ofx_es_member(h, m, 4, 0.05, SEED, 0, _vp(w), _vp(bias)), b"outside"))
    nulls = {"get w": lambda: L.ofx_es_get(h, None, _vp(bias)), "get b": lambda: L.ofx_es_get(h, _vp(w), None),
             "set w": lambda: L.ofx_es_set(h, None, _vp(bias)), "set b": lambda: L.ofx_es_set(h, _vp(w), None),
             "member w": lambda: L.ofx_es_member(h, 1, 4, 0.05, SEED, 0, None, _vp(bias)),
             "member b": lambda: L.ofx_es_member(h, 1, 4, 0.05, SEED, 0, _vp(w), None),
             "act member_of": lambda: L.ofx_es_act(h, None, 4, 0.05, SEED, 0, acts.ptr, None),
             "act actions": lambda: L.ofx_es_act(h, member_of.ptr, 4, 0.05, SEED, 0, None, None),
             "fitness member_of": lambda: L.ofx_es_fitness(h, None, 4, s8.ptr, c4.ptr, 1),
             "fitness sum": lambda: L.ofx_es_fitness(h, member_of.ptr, 4, None, c4.ptr, 1),
             "fitness count": lambda: L.ofx_es_fitness(h, member_of.ptr, 4, s8.ptr, None, 1),
             "update d": lambda: L.ofx_es_update(h, None, 2, 0.1, SEED, 0)}
    for name, call in nulls.items():
        refused.append(("NULL: " + name, call, b"null"))
    for name, call, word in refused:
        assert call() == nat.OFX_ERR_INVALID, name
        assert word in L.ofx_last_error(), (name, L.ofx_last_error())
    assert L.ofx_es_init(None, SEED, 0) == nat.OFX_ERR_INVALID
    b.sync()
    assert np.array_equal(_bits(np.concatenate(b.es_get(nw, nb))), _bits(theta)), "a refused call changed the centre"
    # and the calls as they should be made all go through
    for name, call in calls().items():
        if name not in ("init", "set", "update"):
            assert call() == nat.OFX_OK, name
    b.es_destroy()
    assert L.ofx_es_get(h, _vp(w), _vp(bias)) == nat.OFX_ERR_STATE
    b.es_create(layers)
    b.close()                                                # ofx_destroy frees it


def test_centre_and_population_coexist():
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    from ofighters_amd.evolution import Population
    W, H, P = 48, 40, 3
    layers = [8 + 2 * W * H, 9, 4]
    b = ArenaBatch(1, 1, width=W, height=H)
    pop = Population(b, layers, P, SEED)
    slots = [np.concatenate(b.population_get(p, pop.n_weights, pop.n_biases)) for p in range(P)]
    es = ES(b, layers, SEED + 1)
    assert np.array_equal(_bits(_centre(es)), _bits(eo.fresh(layers, SEED + 1, 0, 0)))
    b.es_update(np.array([1.0, -0.5]), 0.3, SEED + 1, 0)
    _member(es, 1, 4, 0.05, 0)
    for p in range(P):
        got = np.concatenate(b.population_get(p, pop.n_weights, pop.n_biases))
        assert np.array_equal(_bits(got), _bits(slots[p])), "slot %d beside a living centre" % p
    # breeding the population does not touch the centre either
    centre = _centre(es)
    pop.breed(np.array([0, 0, -1], np.int32), 0.05, 0.05, 1)
    assert np.array_equal(_bits(_centre(es)), _bits(centre))
    want = eo.breed(slots, np.array([0, 0, -1]), 0.05, 0.05, SEED, 1, layers)
    es.close()
    for p in range(P):
        got = np.concatenate(b.population_get(p, pop.n_weights, pop.n_biases))
        assert np.array_equal(_bits(got), _bits(want[p])), "slot %d after the centre is gone" % p
    assert np.array_equal(_bits(want[0]), _bits(slots[0]))
    b.close()
