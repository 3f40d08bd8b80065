"""The optimiser of the ES centre on the GPU: ofx_es_step, the moments' export and import, the step statistics, the
checkpoint and the loop, each against tests/es_opt_oracle.py (numpy float64, the contract of include/ofx.h).  theta, m and
v are compared with == on bits everywhere; the three statistics, whose summation order is the library's own, to the worst
case of any order."""
import numpy as np
import pytest

from tests import es_opt_oracle as oo
from tests import es_oracle as so
from tests import evolution_oracle as eo
from tests.es_cases import H, HIDDEN, NIN, SEED, W, bits as _bits, make as _make, same as _same, set_state as _set_state, \
    state as _state, vp as _vp

pytestmark = pytest.mark.gpu

ADAM_SC = dict(gscale=1.0 / (6 * 0.05), alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8)


def _random_moments(G, seed):
    rs = np.random.RandomState(seed)
    m, v = rs.uniform(-0.5, 0.5, G), rs.uniform(0.0, 0.3, G)
    m[:3], v[:3] = [-0.0, 5e-324, 1.0], [0.0, 5e-324, 1.0]
    return m, v


# ---------------------------------------------------------------- 1. the moments cross the layout
@pytest.mark.parametrize("hidden", HIDDEN)
def test_moments_cross_the_layout_and_step(hidden):
    from ofighters_amd import _native as nat
    b, es, layers = _make(hidden, "adam")
    G = eo.n_elements(layers)
    theta = eo.fresh(layers, SEED, 0, 0)
    got = _state(es)
    _same(got, (theta, np.zeros(G), np.zeros(G)), "a fresh optimiser")
    m, v = _random_moments(G, 4)
    es.set_moments(eo.split(layers, m.copy()), eo.split(layers, v.copy()))
    (mW, mB), (vW, vB) = es.moments()
    mo, vo = eo.split(layers, m.copy()), eo.split(layers, v.copy())
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(mW + mB + vW + vB, mo[0] + mo[1] + vo[0] + vo[1]))
    _same(_state(es), (theta, m, v), "set_moments")
    d, generation = np.array([0.4, 0.0, -1.0]), 3
    b.es_step(d, nat.ES_RULE_ADAM, decay=0.005, seed=SEED, generation=generation, **ADAM_SC)
    want = oo.step(theta, m, v, d, oo.ADAM, decay=0.005, seed=SEED, generation=generation, **ADAM_SC)[:3]
    _same(_state(es), want, "one step from imported moments")
    assert (want[0] != theta).mean() > 0.99 and (want[1] != m).mean() > 0.99 and (want[2] != v).mean() > 0.99
    b.close()


# ---------------------------------------------------------------- 2. three consecutive steps
STEPS = [(np.array([0.4, 0.0, -1.0]), 5),                    # a zero weight among the pairs
         (np.zeros(3), 9),                                   # all zeros: theta still moves under decay, m decays
         (np.array([-0.25, 0.75, 0.5]), 2)]


@pytest.mark.parametrize("via", ["raw", "update"])
@pytest.mark.parametrize("decay", [0.0, 0.005])
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
@pytest.mark.parametrize("hidden", HIDDEN)
def test_three_consecutive_steps(hidden, optimizer, decay, via):
    from ofighters_amd import _native as nat
    beta1, beta2, eps, lr, sigma, n_c = 0.8, 0.99, 1e-6, 0.07, 0.05, 6
    b, es, layers = _make(hidden, optimizer, beta1=beta1, beta2=beta2, adam_eps=eps, weight_decay=decay)
    rule = oo.RULES[optimizer]
    assert rule == (nat.ES_RULE_MOMENTUM if optimizer == "momentum" else nat.ES_RULE_ADAM)
    state = _state(es)
    assert not state[1].any() and not state[2].any()
    for t, (d, generation) in enumerate(STEPS, 1):
        gscale, alpha, c1, k1, c2, k2 = oo.scalars(optimizer, lr, sigma, n_c, t, beta1, beta2)
        if via == "raw":
            b.es_step(d, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, SEED, generation)
        else:
            es.update(d, lr, sigma, n_c, generation)
            assert es.opt_steps == t
        want = oo.step(state[0], state[1], state[2], d, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, SEED, generation)[:3]
        got = _state(es)
        _same(got, want, "step %d" % t)
        if not d.any():                                      # q = -decay * theta
            assert (got[1] != state[1]).mean() > 0.99, "all-zero weights did not decay m"
            if decay:
                assert (got[0] != state[0]).mean() > 0.99, "all-zero weights under decay did not move theta"
        if optimizer == "momentum":
            assert not got[2].any(), "momentum wrote v"
        state = got
    b.close()


# ---------------------------------------------------------------- 3. the reference size
def test_step_at_the_reference_size():
    """[320008, 9, 4], 2 pairs, on the element sample of tests/test_gpu_es.py::test_update_at_the_reference_size: the
    first 4096, the last 4096 (second layer and biases), every 997th in between - for theta, m and v, two steps so that
    the second starts from moments the first left."""
    from ofighters_amd import ArenaBatch, _native as nat
    from ofighters_amd.es import ES
    layers = [320008, 9, 4]
    G = eo.n_elements(layers)
    assert G == 2880121
    sample = np.unique(np.concatenate([np.arange(4096), np.arange(4096, G - 4096, 997), np.arange(G - 4096, G)]))
    b = ArenaBatch(1, 1)
    es = ES(b, layers, SEED, optimizer="adam", weight_decay=0.005)
    state = (eo.fresh(layers, SEED, 0, 0, elements=sample), np.zeros(sample.size), np.zeros(sample.size))
    assert not any(x.any() for x in _state(es)[1:]), "the moments do not start at zero"
    for d, generation in ((np.array([0.6, -0.25]), 7), (np.array([-1.0, 0.5]), 8)):
        b.es_step(d, nat.ES_RULE_ADAM, decay=0.005, seed=SEED, generation=generation, **ADAM_SC)
        want = oo.step(state[0], state[1], state[2], d, oo.ADAM, decay=0.005, seed=SEED, generation=generation,
                       elements=sample, **ADAM_SC)[:3]
        got = tuple(x[sample] for x in _state(es))
        _same(got, want, "generation %d" % generation)
        assert all((g != s).mean() > 0.99 for g, s in zip(got, state))
        state = got
    b.close()


# ---------------------------------------------------------------- 4. the statistics
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_stats_fixed_order_and_null(optimizer):
    from ofighters_amd import DeviceBuffer
    b, es, layers = _make((18,), optimizer)
    G = eo.n_elements(layers)
    assert G % 256 != 0 and G > 256 * 256, "the last workgroup is partial and the final pass has more than one round"
    rule = oo.RULES[optimizer]
    theta = eo.fresh(layers, SEED, 0, 0)
    m, v = _random_moments(G, 6)
    d, generation = np.array([0.4, 0.0, -1.0, 0.3]), 4
    want = oo.step(theta, m, v, d, rule, decay=0.005, seed=SEED, generation=generation, **ADAM_SC)
    want_stats = oo.stats(want[0], want[3], want[4])
    sentinel = np.full(3, -7.25)
    runs = []
    for stats in (True, True, False):
        _set_state(es, theta, m, v)
        buf = DeviceBuffer(24).upload(sentinel)
        b.es_step(d, rule, decay=0.005, seed=SEED, generation=generation, stats_ptr=buf.ptr if stats else None, **ADAM_SC)
        b.sync()
        runs.append((_state(es), buf.download(np.float64, (3,))))
        _same(runs[-1][0], want[:3], "stats %s" % stats)
    bound = (G - 1) * 2.0 ** -53
    for k, name in enumerate(("grad_sq", "step_sq", "centre_sq")):
        got = float(runs[0][1][k])
        rel = abs(got - want_stats[k]) / want_stats[k]
        print("%s %s: device %.17g fsum %.17g relative difference %.3e (bound %.3e)" % (optimizer, name, got, want_stats[k],
                                                                                       rel, bound))
        assert want_stats[k] > 0 and rel <= bound, name
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "a second call from the restored state gives other bits"
    assert np.array_equal(_bits(runs[2][1]), _bits(sentinel)), "stats == NULL wrote somewhere"
    # through the Python layer: step_stats() is the last update's
    _set_state(es, theta, m, v)
    es.update(d, 0.03, 0.05, 6, generation)
    assert len(es.step_stats()) == 3 and all(x > 0 for x in es.step_stats())
    b.close()


# ---------------------------------------------------------------- 5. coexistence, refusals, lifetime
def test_update_beside_optimiser_state():
    b, es, layers = _make((9,), "adam")
    G = eo.n_elements(layers)
    theta = eo.fresh(layers, SEED, 0, 0)
    m, v = _random_moments(G, 7)
    _set_state(es, theta, m, v)
    d = np.array([0.4, 0.0, -1.0])
    b.es_update(d, 0.75, SEED, 1)
    _same(_state(es), (so.update(theta, d, 0.75, SEED, 1), m, v), "ofx_es_update beside the moments")
    b.close()


def test_refusals_leave_everything_unchanged():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    L = nat.lib()
    layers = [NIN, 9, 4]
    nw, nb = NIN * 9 + 36, 13
    b = ArenaBatch(1, 1, width=W, height=H)
    h = b.handle
    bufs = [np.zeros(nw), np.zeros(nb), np.zeros(nw), np.zeros(nb)]
    d = np.array([0.5, -0.5])
    ok = dict(rule=2, gscale=3.0, decay=0.005, alpha=0.03, c1=0.9, k1=0.1, c2=0.999, k2=0.001, eps=1e-8)

    def step(d_ptr=_vp(d), n_pairs=2, **kw):
        a = dict(ok, **kw)
        return L.ofx_es_step(h, d_ptr, n_pairs, a["rule"], a["gscale"], a["decay"], a["alpha"], a["c1"], a["k1"], a["c2"],
                             a["k2"], a["eps"], SEED, 0, None)

    def opt_calls():
        return {"opt_destroy": lambda: L.ofx_es_opt_destroy(h), "opt_get": lambda: L.ofx_es_opt_get(h, *map(_vp, bufs)),
                "opt_set": lambda: L.ofx_es_opt_set(h, *map(_vp, bufs)), "step": step}

    # no centre, then a centre without optimiser state: OFX_ERR_STATE, each with its message
    assert L.ofx_es_opt_create(h) == nat.OFX_ERR_STATE and b"no ES centre" in L.ofx_last_error()
    for name, call in opt_calls().items():
        assert call() == nat.OFX_ERR_STATE and b"no ES centre" in L.ofx_last_error(), name
    b.es_create(layers)
    b.es_init(SEED, 0)
    for name, call in opt_calls().items():
        assert call() == nat.OFX_ERR_STATE and b"no optimiser state" in L.ofx_last_error(), name
    b.es_opt_create()
    with pytest.raises(OfxError, match="already") as e:
        b.es_opt_create()
    assert e.value.code == nat.OFX_ERR_STATE
    assert L.ofx_es_opt_create(None) == nat.OFX_ERR_INVALID

    rs = np.random.RandomState(9)
    m, v = rs.uniform(-1, 1, nw + nb), rs.uniform(0, 1, nw + nb)
    b.es_opt_set(m[:nw], m[nw:], v[:nw], v[nw:])
    theta = np.concatenate(b.es_get(nw, nb))
    nan, inf = float("nan"), float("inf")
    refused = [("NULL d", lambda: step(d_ptr=None), b"null"), ("n_pairs = 0", lambda: step(n_pairs=0), b"n_pairs"),
               ("n_pairs = 2^30", lambda: step(n_pairs=1 << 30), b"n_pairs"),
               ("decay < 0", lambda: step(decay=-0.005), b"decay"), ("eps = 0", lambda: step(eps=0.0), b"eps"),
               ("eps < 0", lambda: step(eps=-1e-8), b"eps")]
    for rule in (0, 3, -1):
        refused.append(("rule %d" % rule, lambda rule=rule: step(rule=rule), b"rule"))
    for name in ("gscale", "decay", "alpha", "c1", "k1", "c2", "k2", "eps"):
        for bad in (nan, inf, -inf):
            for rule in (1, 2):
                refused.append(("%s = %r, rule %d" % (name, bad, rule),
                                lambda name=name, bad=bad, rule=rule: step(**{name: bad, "rule": rule}), name.encode()))
    for bad in (nan, inf):
        bad_d = np.array([0.5, bad])
        refused.append(("d[1] = %r" % bad, lambda bad_d=bad_d: step(d_ptr=_vp(bad_d)), b"d[1]"))
    for i in range(4):
        args = [_vp(x) for x in bufs]
        args[i] = None
        refused.append(("opt_get NULL %d" % i, lambda args=args: L.ofx_es_opt_get(h, *args), b"null"))
        refused.append(("opt_set NULL %d" % i, lambda args=args: L.ofx_es_opt_set(h, *args), b"null"))
    for name, call, word in refused:
        assert call() == nat.OFX_ERR_INVALID, name
        assert word in L.ofx_last_error(), (name, L.ofx_last_error())
    b.sync()
    got_m, got_v = b.es_opt_get(nw, nb)
    _same((np.concatenate(b.es_get(nw, nb)), np.concatenate(got_m), np.concatenate(got_v)), (theta, m, v),
          "after the refused calls")
    # momentum does not look at eps's sign, and the calls as they should be made go through
    assert step(rule=1, eps=0.0) == nat.OFX_OK and step() == nat.OFX_OK
    b.sync()
    b.close()


def test_lifetime():
    from ofighters_amd import OfxError, _native as nat
    b, es, layers = _make((9,), "momentum")
    G = eo.n_elements(layers)
    d = np.array([1.0, -0.5])
    es.update(d, 0.1, 0.05, 4, 0)
    theta, m, v = _state(es)
    assert m.any() and not v.any()
    b.es_opt_destroy()
    with pytest.raises(OfxError) as e:
        b.es_opt_get(es.n_weights, es.n_biases)
    assert e.value.code == nat.OFX_ERR_STATE
    assert np.array_equal(_bits(np.concatenate(b.es_get(es.n_weights, es.n_biases))), _bits(theta)), "destroy moved the centre"
    b.es_opt_create()                                        # again: zeroed
    _same(_state(es), (theta, np.zeros(G), np.zeros(G)), "created again")
    b.es_destroy()                                           # frees the moments with the centre
    b.es_create(layers)
    with pytest.raises(OfxError) as e:
        b.es_opt_get(es.n_weights, es.n_biases)
    assert e.value.code == nat.OFX_ERR_STATE
    b.es_opt_create()
    b.es_init(SEED, 0)
    _same(_state(es), (eo.fresh(layers, SEED, 0, 0), np.zeros(G), np.zeros(G)), "a new centre")
    b.close()                                                # ofx_destroy frees all of it


# ---------------------------------------------------------------- 6. the loop
LOOP = dict(N=8, M=3, P=4, W=48, H=40, T=10, sigma=0.05, lr=0.2, eval_arenas=2)      # tests/test_gpu_es.py's sizes
OPT = dict(optimizer="adam", weight_decay=0.005)


def _rollout(seed, init=True):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES, ESRollout
    L = LOOP
    layers = [8 + 2 * L["W"] * L["H"], 9, 4]
    b = ArenaBatch(L["N"], L["M"], width=L["W"], height=L["H"])
    es = ES(b, layers, seed, init=init, **OPT)
    roll = ESRollout(b, es, ["random"] * L["M"], seed, L["P"], L["sigma"], L["lr"], ships=(0,),
                     eval_arenas=L["eval_arenas"], episode_ticks=L["T"], log_steps=True)
    return b, es, roll


def _loop(seed):
    b, es, roll = _rollout(seed)
    T = LOOP["T"]
    snaps = [_state(es)]
    for _ in range(3):
        roll.run(T + (1 if len(snaps) == 1 else 0))      # up to and including the lock-step that ends a generation
        snaps.append(_state(es))
    out = dict(fitness_log=list(roll.fitness_log), centre_log=list(roll.centre_log), weight_log=list(roll.weight_log),
               step_log=list(roll.step_log), snaps=snaps, generation=roll.generation, tick=roll.tick, opt_steps=es.opt_steps)
    b.close()
    return out


@pytest.fixture(scope="module")
def loop_run():
    return _loop(oo.LOOP_SEED)


def test_es_optimizer_loop_on_the_device(loop_run):
    r1, r2 = loop_run, _loop(oo.LOOP_SEED)
    L = LOOP
    layers = [8 + 2 * L["W"] * L["H"], 9, 4]
    G = eo.n_elements(layers)
    assert r1["generation"] == 3 and len(r1["weight_log"]) == len(r1["step_log"]) == 3 == r1["opt_steps"]
    assert r1["fitness_log"] == r2["fitness_log"] and r1["centre_log"] == r2["centre_log"]
    assert r1["step_log"] == r2["step_log"], "two runs' statistics differ"
    for g, (s1, s2) in enumerate(zip(r1["snaps"], r2["snaps"])):
        _same(s1, s2, "two runs, after %d generations" % g)
    assert r1["weight_log"][0][0].any(), "generation 0 of this seed has no untied pair: the first step saw no estimate"
    # every generation's centre and moments are the oracle's step from the previous ones with the recorded weights
    for gen, (d, n_c) in enumerate(r1["weight_log"]):
        assert n_c == L["P"], "six learning arenas fly all four members"
        gscale, alpha, c1, k1, c2, k2 = oo.scalars("adam", L["lr"], L["sigma"], n_c, gen + 1, 0.9, 0.999)
        old = r1["snaps"][gen]
        want = oo.step(old[0], old[1], old[2], d, oo.ADAM, gscale, 0.005, alpha, c1, k1, c2, k2, 1e-8, oo.LOOP_SEED, gen)
        _same(r1["snaps"][gen + 1], want[:3], "generation %d" % gen)
        for got, w in zip(r1["step_log"][gen], oo.stats(want[0], want[3], want[4])):
            assert abs(got - w) <= (G - 1) * 2.0 ** -53 * w
    print("weights per generation:", [(list(d), n) for d, n in r1["weight_log"]], "step_log:", r1["step_log"])


def test_es_optimizer_loop_resumes_bit_for_bit(loop_run, tmp_path):
    T = LOOP["T"]
    b, es, roll = _rollout(oo.LOOP_SEED)
    roll.run(T + 4)                                      # inside the second generation's episode
    path = es.save(str(tmp_path / "centre.npy"))
    state = roll.state_dict()
    assert state["generation"] == 1 and es.opt_steps == 1 and len(state["step_log"]) == 1
    _same(_state(es), loop_run["snaps"][1], "before the stop")
    b.close()
    b3, es3, roll3 = _rollout(oo.LOOP_SEED, init=False)  # fresh handles
    es3.load(path)
    assert es3.opt_steps == 1
    _same(_state(es3), loop_run["snaps"][1], "after ES.load")
    roll3.load_state_dict(state)
    roll3.run(loop_run["tick"] - (T + 4))
    assert roll3.generation == 3 and roll3.tick == loop_run["tick"] and es3.opt_steps == 3
    assert roll3.fitness_log == loop_run["fitness_log"] and roll3.centre_log == loop_run["centre_log"]
    assert roll3.step_log == loop_run["step_log"]
    _same(_state(es3), loop_run["snaps"][3], "the resumed run")
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(roll3.weight_log, loop_run["weight_log"]))
    b3.close()
    # an ES without the optimiser refuses the checkpoint, untouched
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    b4 = ArenaBatch(1, 1, width=LOOP["W"], height=LOOP["H"])
    plain = ES(b4, [8 + 2 * LOOP["W"] * LOOP["H"], 9, 4], oo.LOOP_SEED)
    before = np.concatenate(b4.es_get(plain.n_weights, plain.n_biases))
    with pytest.raises(ValueError, match="optimizer"):
        plain.load(path)
    assert np.array_equal(_bits(np.concatenate(b4.es_get(plain.n_weights, plain.n_biases))), _bits(before))
    b4.close()
