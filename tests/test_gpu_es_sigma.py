"""Per-element adaptive sigma of the ES centre on the GPU: the sigma vector's layout, members, the forward, the
generation step of centre and sigma, its statistics, the refusals, the lifetime and the loop, each against
tests/es_sigma_oracle.py (numpy float64, the contract of include/ofx.h).  Every comparison of state - theta, sigma, m, v,
y, the five statistics - is == on bits; only the numpy forward is compared at rtol 1e-12."""
import numpy as np
import pytest

from tests import es_opt_oracle as oo
from tests import es_oracle as so
from tests import es_sigma_oracle as sg
from tests import es_cases
from tests import evolution_oracle as eo
from tests.es_cases import H, HIDDEN, NIN, SEED, W, bits as _bits, same as _same, set_state as _set_state, \
    state as _state, vp as _vp
from tests.test_gpu_es import _assignment, _scaled_genome, _scene

pytestmark = pytest.mark.gpu

OPTIMIZERS = [None, "momentum", "adam"]


def _make(hidden, optimizer=None, sigma_init=0.05, **kw):
    """es_cases.make with adaptation on"""
    return es_cases.make(hidden, optimizer, sigma_init=sigma_init, **kw)


def _distinct_sigma(G):
    """Every element another width, in [0.01, 0.09): the index is readable from the value."""
    return 0.01 + np.arange(G, dtype=np.float64) * (0.08 / G)


def _zeros_if_none(x, like):
    return np.zeros_like(like) if x is None else x


# ---------------------------------------------------------------- 1. the sigma vector crosses the layout; members
@pytest.mark.parametrize("hidden", HIDDEN)
def test_sigma_crosses_the_layout_and_members(hidden):
    b, es, layers = _make(hidden, sigma_init=0.07)
    G = eo.n_elements(layers)
    theta = eo.fresh(layers, SEED, 0, 0)
    _same(_state(es), (theta, np.full(G, 0.07), None, None), "a fresh vector")
    sigma = _distinct_sigma(G)
    assert np.unique(sigma).size == G
    es.set_sigmas(*eo.split(layers, sigma.copy()))
    Wl, Bl = es.sigmas()
    Wo, Bo = eo.split(layers, sigma.copy())
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(Wl + Bl, Wo + Bo))
    _same(_state(es), (theta, sigma, None, None), "set_sigmas")
    P, generation = 6, 3
    for m in (0, 1, 3, P):
        got = np.concatenate(b.es_sigma_member(m, P, SEED, generation, es.n_weights, es.n_biases))
        want = sg.member(theta, sigma, SEED, m, P, generation)
        assert np.array_equal(_bits(got), _bits(want)), "member %d" % m
    Wl, Bl = es.member(3, P, None, generation)
    Wo, Bo = eo.split(layers, sg.member(theta, sigma, SEED, 3, P, generation))
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(Wl + Bl, Wo + Bo))
    _same(_state(es), (theta, sigma, None, None), "materialising members")
    b.close()


# ---------------------------------------------------------------- 2. a uniform vector is the scalar law
@pytest.mark.parametrize("hidden", HIDDEN)
def test_uniform_sigma_equals_the_scalar_calls(hidden):
    from ofighters_amd import DeviceBuffer
    N, M, P, sigma, generation = 3, 3, 4, 0.02, 5
    b, es, layers = _make(hidden, sigma_init=sigma, N=N, M=M)
    _scene(b, SEED)
    es.set_centre(*_scaled_genome(layers, np.random.RandomState(3)))
    nw, nb = es.n_weights, es.n_biases
    for m in range(P + 1):
        got = np.concatenate(b.es_sigma_member(m, P, SEED, generation, nw, nb))
        assert np.array_equal(_bits(got), _bits(np.concatenate(b.es_member(m, P, sigma, SEED, generation, nw, nb)))), m
    member_of = _assignment(N, M, P)
    es.assign(member_of, P)
    sentinel = np.full((N, M, 4), -7.25)
    out = []
    for adaptive in (False, True):
        dy = DeviceBuffer(sentinel.nbytes).upload(sentinel)
        b.bot_actions(["random"] * M, SEED, tick=100)
        if adaptive:
            es.act(None, generation, y_ptr=dy.ptr)
        else:
            b.es_act(es._member_of.ptr, P, sigma, SEED, generation, y_ptr=dy.ptr)
        b.sync()
        out.append((dy.download(np.float64, (N, M, 4)), b.actions_host()))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])), "y under a uniform vector is not ofx_es_act's"
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert (out[1][0] != sentinel).any() and (out[1][0] == sentinel).any()
    b.close()


# ---------------------------------------------------------------- 3. the forward equals the stored-genome forward
FORWARD_CASES = [(48, 40, M, hidden) for M in (3, 13) for hidden in HIDDEN] + [(400, 400, 3, (9,))]


@pytest.mark.parametrize("W_,H_,M,hidden", FORWARD_CASES)
def test_forward_equals_the_stored_genome_forward(W_, H_, M, hidden):
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from ofighters_amd.es import ES
    from ofighters_amd.evolution import Population
    big = W_ == 400
    N, P = (2, 2) if big else (3, 4)
    generation = 5
    layers = [8 + 2 * W_ * H_] + list(hidden) + [4]
    G = eo.n_elements(layers)
    b = ArenaBatch(N, M, width=W_, height=H_)
    _scene(b, SEED)
    es = ES(b, layers, SEED, sigma_init=0.02)
    pop = Population(b, layers, P + 1, SEED)                 # on the same handle: slot m holds member m, slot P the centre
    es.set_centre(*_scaled_genome(layers, np.random.RandomState(3)))
    sigma = np.random.RandomState(6).uniform(0.005, 0.04, G)
    es.set_sigmas(*eo.split(layers, sigma.copy()))
    theta = np.concatenate(b.es_get(es.n_weights, es.n_biases))
    member_of = _assignment(N, M, P)
    es.assign(member_of, P)
    pop.assign(member_of)
    alive = b.get(nat.F_SHIP_ALIVE)
    flown = (member_of >= 0) & (alive != 0)
    assert not flown[N - 1, 1] and member_of[N - 1, 1] >= 0 and flown.sum() >= 3
    assert {0, 1, P} <= set(int(v) for v in member_of[flown]), "both signs of pair 0 and the centre fly"
    want_member = {}
    for m in (int(v) for v in np.unique(member_of[flown])):
        got = np.concatenate(b.es_sigma_member(m, P, SEED, generation, es.n_weights, es.n_biases))
        want_member[m] = sg.member(theta, sigma, SEED, m, P, generation)
        assert np.array_equal(_bits(got), _bits(want_member[m])), "member %d" % m
        pop.set_genome(m, *eo.split(layers, got))
    assert not np.array_equal(want_member[0], so.member(theta, SEED, 0, P, 0.02, generation)), "the vector is not in play"

    sentinel = np.full((N, M, 4), -7.25)
    dy_pop, dy_es = DeviceBuffer(sentinel.nbytes).upload(sentinel), DeviceBuffer(sentinel.nbytes).upload(sentinel)
    b.bot_actions(["random"] * M, SEED, tick=100)
    before = b.actions_host()
    pop.act(y_ptr=dy_pop.ptr)
    b.sync()
    y_pop, act_pop = dy_pop.download(np.float64, (N, M, 4)), b.actions_host()
    b.bot_actions(["random"] * M, SEED, tick=100)
    assert b.actions_host().tobytes() == before.tobytes()
    es.act(None, generation, y_ptr=dy_es.ptr)
    b.sync()
    y, act_es = dy_es.download(np.float64, (N, M, 4)), b.actions_host()
    es.act(None, generation, y_ptr=dy_es.ptr)
    b.sync()
    assert np.array_equal(_bits(y), _bits(dy_es.download(np.float64, (N, M, 4)))), "a second call gives other bits"
    assert act_es.tobytes() == b.actions_host().tobytes()

    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_F64)
    for a in range(N):
        for i in range(M):
            if not flown[a, i]:                              # dead, unassigned: neither y nor the action is written
                assert np.array_equal(y[a, i], sentinel[a, i])
                assert act_es[a, i].tobytes() == before[a, i].tobytes()
                continue
            m = int(member_of[a, i])
            assert np.array_equal(_bits(y[a, i]), _bits(y_pop[a, i])), "arena %d ship %d member %d: y" % (a, i, m)
            assert act_es[a, i].tobytes() == act_pop[a, i].tobytes(), "arena %d ship %d member %d: action" % (a, i, m)
            want = eo.forward(layers, want_member[m], head[a, i], sm[a], lm[a])
            print("case %dx%d M=%d %s arena %d ship %d member %d: max rel err against numpy %.3e"
                  % (W_, H_, M, hidden, a, i, m, np.max(np.abs(y[a, i] - want) / np.abs(want))))
            np.testing.assert_allclose(y[a, i], want, rtol=1e-12, atol=0)
    _same(_state(es), (theta, sigma, None, None), "acting")
    b.close()


# ---------------------------------------------------------------- 4. three consecutive steps
# pair 0: both weights; pair 1: d = 0, s != 0 (a tied pair above the baseline); pair 2: d != 0, s = 0; pair 3: both zero
STEPS = [(np.array([0.4, 0.0, -1.0, 0.0, 0.25]), np.array([0.3, 0.5, 0.0, 0.0, -0.8]), 5),
         (np.array([0.0, 0.0, 0.0, 0.0, 0.0]), np.array([0.0, -0.6, 0.0, 0.0, 0.6]), 9),    # d all zero: decay and sigma move
         (np.array([-0.25, 0.0, 0.5, 0.0, 0.75]), np.array([-0.5, 0.25, 0.0, 0.0, 0.25]), 2)]
CLAMP = dict(sigma_init=0.05, sigma_lr=3.0, sigma_min=0.04, sigma_max=0.065)                # srate 0.3 at n_c = 10


@pytest.mark.parametrize("via", ["raw", "update"])
@pytest.mark.parametrize("decay", [0.0, 0.005])
@pytest.mark.parametrize("optimizer", OPTIMIZERS)
@pytest.mark.parametrize("hidden", HIDDEN)
def test_three_consecutive_steps(hidden, optimizer, decay, via):
    from ofighters_amd import _native as nat
    beta1, beta2, eps, lr, n_c = 0.8, 0.99, 1e-6, 0.07, 10
    b, es, layers = _make(hidden, optimizer, beta1=beta1, beta2=beta2, adam_eps=eps, weight_decay=decay, **CLAMP)
    rule = sg.RULES[optimizer]
    assert rule == {None: nat.ES_RULE_PLAIN, "momentum": nat.ES_RULE_MOMENTUM, "adam": nat.ES_RULE_ADAM}[optimizer]
    state = _state(es)
    smin, smax = CLAMP["sigma_min"], CLAMP["sigma_max"]
    for t, (d, s, generation) in enumerate(STEPS, 1):
        gscale, alpha, c1, k1, c2, k2, srate = sg.scalars(optimizer, lr, n_c, t, beta1, beta2, CLAMP["sigma_lr"])
        m0, v0 = _zeros_if_none(state[2], state[0]), _zeros_if_none(state[3], state[0])
        want = sg.step(state[0], state[1], m0, v0, d, s, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax,
                       SEED, generation)
        # by the oracle alone: some elements hit each clamp, most hit neither
        low, high = want[1] == smin, want[1] == smax
        assert 0 < low.mean() and 0 < high.mean() and (low | high).mean() < 0.5, (t, low.mean(), high.mean())
        assert want[6].sum() > 0 and (want[1] != state[1]).mean() > 0.9
        if via == "raw":
            b.es_sigma_step(d, s, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax, SEED, generation)
        else:
            es.update(d, lr, None, n_c, generation, s=s)
            assert es.opt_steps == (t if optimizer else 0)
        got = _state(es)
        want_state = (want[0], want[1], want[2] if optimizer else None, want[3] if optimizer else None)
        _same(got, want_state, "step %d" % t)
        if d.any() or decay:
            assert (got[0] != state[0]).mean() > 0.99, "theta did not move"
        else:
            moved = (got[0] != state[0]).mean()
            assert moved == 0 if optimizer is None else moved > 0.99, "d = 0 without decay: only the moments step"
        if optimizer == "momentum":
            assert not got[3].any(), "momentum wrote v"
        state = got
    b.close()


# ---------------------------------------------------------------- 5. the degenerate equalities on the device
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_unit_sigma_and_zero_rate_equal_ofx_es_step(optimizer):
    """sigma = 1 and srate = 0: theta', m', v' are ofx_es_step's on a second handle; sigma stays 1."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    b, es, layers = _make((13, 7), optimizer, sigma_init=1.0, sigma_min=0.5, sigma_max=2.0)
    b2 = ArenaBatch(1, 1, width=W, height=H)
    ref = ES(b2, layers, SEED, optimizer=optimizer)
    G = eo.n_elements(layers)
    rule = sg.RULES[optimizer]
    sc = dict(gscale=1.0 / 6, decay=0.005, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8)
    for d, s, generation in STEPS:
        b.es_sigma_step(d, s, rule, srate=0.0, smin=0.5, smax=2.0, seed=SEED, generation=generation, **sc)
        b2.es_step(d, rule, seed=SEED, generation=generation, **sc)
        got = _state(es)
        m, v = b2.es_opt_get(ref.n_weights, ref.n_biases)
        _same(got, (np.concatenate(b2.es_get(ref.n_weights, ref.n_biases)), np.ones(G), np.concatenate(m), np.concatenate(v)),
              "generation %d" % generation)
    assert (got[0] != eo.fresh(layers, SEED, 0, 0)).mean() > 0.99
    b.close()
    b2.close()


@pytest.mark.parametrize("optimizer", OPTIMIZERS)
def test_zero_utilities_leave_sigma(optimizer):
    b, es, layers = _make((9,), optimizer, sigma_min=0.005, sigma_max=0.1)
    G = eo.n_elements(layers)
    sigma = _distinct_sigma(G)
    sigma[:3] = [0.005, 0.1, 0.05]                           # the clamp's own values are inside it
    es.set_sigmas(*eo.split(layers, sigma.copy()))
    theta = eo.fresh(layers, SEED, 0, 0)
    d = np.array([0.4, 0.0, -1.0])
    for srate in (0.3, -7.5, 1e300):
        b.es_sigma_step(d, np.zeros(3), sg.RULES[optimizer], 1.0 / 6, 0.0, 0.03, 0.9, 0.1, 0.999, 0.001, 1e-8, srate, 0.005,
                        0.1, SEED, 4)
        got = _state(es)
        assert np.array_equal(_bits(got[1]), _bits(sigma)), "s = 0 moved sigma at srate %r" % srate
    assert (got[0] != theta).mean() > 0.99
    b.close()


# ---------------------------------------------------------------- 6. the statistics
@pytest.mark.parametrize("optimizer", OPTIMIZERS)
def test_stats_fixed_order_and_null(optimizer):
    from ofighters_amd import DeviceBuffer
    b, es, layers = _make((18,), optimizer, **CLAMP)
    G = eo.n_elements(layers)
    assert G % 256 != 0 and G > 256 * 256, "the last workgroup is partial and the final pass has more than one round"
    rule = sg.RULES[optimizer]
    rs = np.random.RandomState(6)
    theta, sigma = eo.fresh(layers, SEED, 0, 0), rs.uniform(0.041, 0.064, G)
    m, v = (rs.uniform(-0.5, 0.5, G), rs.uniform(0.0, 0.3, G)) if optimizer else (None, None)
    d, s, generation = STEPS[0]
    sc = dict(gscale=1.0 / 10, decay=0.005, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8, srate=0.3,
              smin=0.04, smax=0.065)
    want = sg.step(theta, sigma, _zeros_if_none(m, theta), _zeros_if_none(v, theta), d, s, rule, seed=SEED,
                   generation=generation, **sc)
    want_state = (want[0], want[1], want[2] if optimizer else None, want[3] if optimizer else None)
    want_stats = sg.stats(want[0], want[1], want[4], want[5], want[6], layers)
    assert 0 < want_stats[4] < G / 2 and want_stats[4] == want[6].sum()
    sentinel = np.full(5, -7.25)
    runs = []
    for stats in (True, True, False):
        _set_state(es, theta, sigma, m, v)
        buf = DeviceBuffer(40).upload(sentinel)
        b.es_sigma_step(d, s, rule, seed=SEED, generation=generation, stats_ptr=buf.ptr if stats else None, **sc)
        b.sync()
        runs.append((_state(es), buf.download(np.float64, (5,))))
        _same(runs[-1][0], want_state, "stats %s" % stats)
    for k, name in enumerate(("grad_sq", "step_sq", "centre_sq", "sigma_sq", "clamped")):
        print("%s %s: device %.17g oracle %.17g" % (optimizer, name, runs[0][1][k], want_stats[k]))
    assert np.array_equal(_bits(runs[0][1]), _bits(np.array(want_stats))), "the five sums are not the fixed order's"
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "a second call from the restored state gives other bits"
    assert np.array_equal(_bits(runs[2][1]), _bits(sentinel)), "stats == NULL wrote somewhere"
    _set_state(es, theta, sigma, m, v)                       # through the Python layer: step_stats() is the last update's
    es.update(d, 0.03, None, 10, generation, s=s)
    assert len(es.step_stats()) == 5 and all(x > 0 for x in es.step_stats())
    b.close()


# ---------------------------------------------------------------- 7. the reference size
def test_member_and_step_at_the_reference_size():
    """[320008, 9, 4], 2 pairs, on the element sample of tests/test_gpu_es.py::test_update_at_the_reference_size: the
    first 4096, the last 4096 (second layer and biases), every 997th in between - a distinct sigma across the
    input-major / element-order mapping at full size, a member, and two Adam steps of theta, sigma, m and v."""
    from ofighters_amd import ArenaBatch, _native as nat
    from ofighters_amd.es import ES
    layers = [320008, 9, 4]
    G = eo.n_elements(layers)
    assert G == 2880121
    sample = np.unique(np.concatenate([np.arange(4096), np.arange(4096, G - 4096, 997), np.arange(G - 4096, G)]))
    b = ArenaBatch(1, 1)
    es = ES(b, layers, SEED, optimizer="adam", weight_decay=0.005, sigma_init=0.05)
    full = _distinct_sigma(G)
    nw = es.n_weights
    b.es_sigma_set(full[:nw], full[nw:])
    pick = lambda st: tuple(x[sample] for x in st)
    state = (eo.fresh(layers, SEED, 0, 0, elements=sample), full[sample], np.zeros(sample.size), np.zeros(sample.size))
    _same(pick(_state(es)), state, "the start")
    got = np.concatenate(b.es_sigma_member(3, 4, SEED, 7, es.n_weights, es.n_biases))[sample]
    assert np.array_equal(_bits(got), _bits(sg.member(state[0], state[1], SEED, 3, 4, 7, elements=sample)))
    sc = dict(gscale=1.0 / 4, decay=0.005, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8, srate=0.5,
              smin=0.009, smax=0.095)
    for d, s, generation in ((np.array([0.6, -0.25]), np.array([0.4, -0.4]), 7), (np.array([-1.0, 0.5]), np.array([0.0, 0.7]), 8)):
        b.es_sigma_step(d, s, nat.ES_RULE_ADAM, seed=SEED, generation=generation, **sc)
        want = sg.step(*state, d, s, sg.ADAM, seed=SEED, generation=generation, elements=sample, **sc)
        got = pick(_state(es))
        _same(got, want[:4], "generation %d" % generation)
        assert all((g != w).mean() > 0.9 for g, w in zip(got, state))
        state = got
    b.close()


# ---------------------------------------------------------------- 8. refusals, coexistence, lifetime
def test_refusals_leave_everything_unchanged():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    L = nat.lib()
    layers = [NIN, 9, 4]
    nw, nb = NIN * 9 + 36, 13
    b = ArenaBatch(2, 2, width=W, height=H)
    h = b.handle
    w, bias = np.full(nw, 0.05), np.full(nb, 0.05)
    member_of = DeviceBuffer(16).upload(np.array([[0, 1], [2, -1]], np.int32))
    acts = DeviceBuffer(12 * 4)
    d, s = np.array([0.5, -0.5]), np.array([0.25, 0.0])
    ok = dict(rule=2, gscale=0.25, decay=0.005, alpha=0.03, c1=0.9, k1=0.1, c2=0.999, k2=0.001, eps=1e-8, srate=0.1,
              smin=0.01, smax=0.2)

    def step(d_ptr=_vp(d), s_ptr=_vp(s), n_pairs=2, **kw):
        a = dict(ok, **kw)
        return L.ofx_es_sigma_step(h, d_ptr, s_ptr, n_pairs, a["rule"], a["gscale"], a["decay"], a["alpha"], a["c1"], a["k1"],
                                   a["c2"], a["k2"], a["eps"], a["srate"], a["smin"], a["smax"], SEED, 0, None)

    def calls(P=4):
        return {"destroy": lambda: L.ofx_es_sigma_destroy(h), "get": lambda: L.ofx_es_sigma_get(h, _vp(w), _vp(bias)),
                "set": lambda: L.ofx_es_sigma_set(h, _vp(w), _vp(bias)),
                "member": lambda: L.ofx_es_sigma_member(h, 1, P, SEED, 0, _vp(w), _vp(bias)),
                "act": lambda: L.ofx_es_sigma_act(h, member_of.ptr, P, SEED, 0, acts.ptr, None), "step": step}

    # no centre, then a centre without a vector: OFX_ERR_STATE, each with its message
    assert L.ofx_es_sigma_create(h, 0.05) == nat.OFX_ERR_STATE and b"no ES centre" in L.ofx_last_error()
    for name, call in calls().items():
        assert call() == nat.OFX_ERR_STATE and b"no ES centre" in L.ofx_last_error(), name
    b.es_create(layers)
    b.es_init(SEED, 0)
    b.spawn_random(SEED)
    for name, call in calls().items():
        assert call() == nat.OFX_ERR_STATE and b"no sigma vector" in L.ofx_last_error(), name
    for bad in (0.0, -0.05, float("nan"), float("inf")):
        assert L.ofx_es_sigma_create(h, bad) == nat.OFX_ERR_INVALID and b"sigma0" in L.ofx_last_error(), bad
        assert L.ofx_es_sigma_get(h, _vp(w), _vp(bias)) == nat.OFX_ERR_STATE, "a refused create left a vector"
    b.es_sigma_create(0.05)
    with pytest.raises(OfxError, match="already") as e:
        b.es_sigma_create(0.05)
    assert e.value.code == nat.OFX_ERR_STATE
    assert L.ofx_es_sigma_create(None, 0.05) == nat.OFX_ERR_INVALID
    # MOMENTUM and ADAM need the moments; PLAIN does not
    for rule in (1, 2):
        assert step(rule=rule) == nat.OFX_ERR_STATE and b"no optimiser state" in L.ofx_last_error()
    b.es_opt_create()

    rs = np.random.RandomState(9)
    G = nw + nb
    m, v, sigma = rs.uniform(-1, 1, G), rs.uniform(0, 1, G), rs.uniform(0.02, 0.1, G)
    b.es_opt_set(m[:nw], m[nw:], v[:nw], v[nw:])
    b.es_sigma_set(sigma[:nw], sigma[nw:])
    theta = np.concatenate(b.es_get(nw, nb))
    nan, inf = float("nan"), float("inf")
    refused = [("NULL d", lambda: step(d_ptr=None), b"null"), ("NULL s", lambda: step(s_ptr=None), b"null"),
               ("n_pairs = 0", lambda: step(n_pairs=0), b"n_pairs"), ("n_pairs = 2^30", lambda: step(n_pairs=1 << 30), b"n_pairs"),
               ("decay < 0", lambda: step(decay=-0.005), b"decay"), ("eps = 0", lambda: step(eps=0.0), b"eps"),
               ("eps < 0", lambda: step(eps=-1e-8), b"eps"), ("smin = 0", lambda: step(smin=0.0), b"smin"),
               ("smin < 0", lambda: step(smin=-0.01), b"smin"), ("smax < smin", lambda: step(smin=0.1, smax=0.05), b"smax")]
    for rule in (3, -1):
        refused.append(("rule %d" % rule, lambda rule=rule: step(rule=rule), b"rule"))
    for name in ("gscale", "decay", "alpha", "c1", "k1", "c2", "k2", "eps", "srate", "smin", "smax"):
        for bad in (nan, inf, -inf):
            for rule in (0, 1, 2):
                refused.append(("%s = %r, rule %d" % (name, bad, rule),
                                lambda name=name, bad=bad, rule=rule: step(**{name: bad, "rule": rule}), name.encode()))
    for bad in (nan, inf):
        arr = np.array([0.5, bad])
        refused.append(("d[1] = %r" % bad, lambda arr=arr: step(d_ptr=_vp(arr)), b"d[1]"))
        refused.append(("s[1] = %r" % bad, lambda arr=arr: step(s_ptr=_vp(arr)), b"s[1]"))
    for i, bad in ((5, 0.0), (nw - 1, -0.05), (7, nan), (9, inf)):
        bw = w.copy()
        bw[i] = bad
        refused.append(("set weights[%d] = %r" % (i, bad), lambda bw=bw: L.ofx_es_sigma_set(h, _vp(bw), _vp(bias)),
                        ("sigma[%d]" % i).encode()))
    bb = bias.copy()
    bb[2] = 0.0
    refused.append(("set biases[2] = 0", lambda: L.ofx_es_sigma_set(h, _vp(w), _vp(bb)), ("sigma[%d]" % (nw + 2)).encode()))
    for P in (3, 1, 0, -2):
        for name in ("member", "act"):
            refused.append(("P = %d, %s" % (P, name), calls(P=P)[name], b"P must"))
    for mm in (-1, 5):
        refused.append(("member %d" % mm, lambda mm=mm: L.ofx_es_sigma_member(h, mm, 4, SEED, 0, _vp(w), _vp(bias)), b"outside"))
    nulls = {"get w": lambda: L.ofx_es_sigma_get(h, None, _vp(bias)), "get b": lambda: L.ofx_es_sigma_get(h, _vp(w), None),
             "set w": lambda: L.ofx_es_sigma_set(h, None, _vp(bias)), "set b": lambda: L.ofx_es_sigma_set(h, _vp(w), None),
             "member w": lambda: L.ofx_es_sigma_member(h, 1, 4, SEED, 0, None, _vp(bias)),
             "member b": lambda: L.ofx_es_sigma_member(h, 1, 4, SEED, 0, _vp(w), None),
             "act member_of": lambda: L.ofx_es_sigma_act(h, None, 4, SEED, 0, acts.ptr, None),
             "act actions": lambda: L.ofx_es_sigma_act(h, member_of.ptr, 4, SEED, 0, None, None)}
    for name, call in nulls.items():
        refused.append(("NULL: " + name, call, b"null"))
    for name, call, word in refused:
        assert call() == nat.OFX_ERR_INVALID, name
        assert word in L.ofx_last_error(), (name, L.ofx_last_error())
    b.sync()

    def state():
        gm, gv = b.es_opt_get(nw, nb)
        return np.concatenate(b.es_get(nw, nb)), np.concatenate(b.es_sigma_get(nw, nb)), np.concatenate(gm), np.concatenate(gv)

    _same(state(), (theta, sigma, m, v), "after the refused calls")
    # PLAIN beside the moments: it reads and writes neither, and does not look at eps
    assert step(rule=0, eps=0.0) == nat.OFX_OK
    got = state()
    want = sg.step(theta, sigma, m, v, d, s, sg.PLAIN, **dict({k: ok[k] for k in ok if k != "rule"}, eps=0.0), seed=SEED,
                   generation=0)
    _same(got, (want[0], want[1], m, v), "a PLAIN step beside the moments")
    assert (got[0] != theta).mean() > 0.99 and (got[1] != sigma).mean() > 0.9
    # and the calls as they should be made all go through
    assert step(rule=1, eps=0.0) == nat.OFX_OK and step() == nat.OFX_OK
    for name, call in calls().items():
        if name not in ("destroy", "set", "step"):
            assert call() == nat.OFX_OK, name
    b.sync()
    b.close()


def test_lifetime_and_the_older_steps_beside_the_vector():
    from ofighters_amd import OfxError, _native as nat
    b, es, layers = _make((9,), "adam", sigma_init=0.05)
    G = eo.n_elements(layers)
    nw, nb = es.n_weights, es.n_biases
    sigma = _distinct_sigma(G)
    es.set_sigmas(*eo.split(layers, sigma.copy()))
    theta = eo.fresh(layers, SEED, 0, 0)
    d = np.array([0.4, 0.0, -1.0])
    # ofx_es_update and ofx_es_step work beside the vector and do not touch it
    b.es_update(d, 0.75, SEED, 1)
    theta = so.update(theta, d, 0.75, SEED, 1)
    _same(_state(es), (theta, sigma, np.zeros(G), np.zeros(G)), "ofx_es_update beside the vector")
    sc = dict(gscale=1.0 / 6, decay=0.005, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8)
    b.es_step(d, nat.ES_RULE_ADAM, seed=SEED, generation=2, **sc)
    want = oo.step(theta, np.zeros(G), np.zeros(G), d, oo.ADAM, seed=SEED, generation=2, **sc)
    _same(_state(es), (want[0], sigma, want[1], want[2]), "ofx_es_step beside the vector")
    # destroy / create: the vector alone goes and comes back filled
    b.es_sigma_destroy()
    with pytest.raises(OfxError) as e:
        b.es_sigma_get(nw, nb)
    assert e.value.code == nat.OFX_ERR_STATE and "no sigma vector" in str(e.value)
    assert np.array_equal(_bits(np.concatenate(b.es_get(nw, nb))), _bits(want[0])), "destroy moved the centre"
    b.es_sigma_create(0.125)
    _same(_state(es), (want[0], np.full(G, 0.125), want[1], want[2]), "created again")
    b.es_opt_destroy()                                       # the moments go, the vector stays
    assert np.array_equal(_bits(np.concatenate(b.es_sigma_get(nw, nb))), _bits(np.full(G, 0.125)))
    b.es_destroy()                                           # frees the vector with the centre
    b.es_create(layers)
    with pytest.raises(OfxError) as e:
        b.es_sigma_get(nw, nb)
    assert e.value.code == nat.OFX_ERR_STATE
    b.es_sigma_create(0.03)
    b.es_init(SEED, 0)
    assert np.array_equal(_bits(np.concatenate(b.es_sigma_get(nw, nb))), _bits(np.full(G, 0.03)))
    assert np.array_equal(_bits(np.concatenate(b.es_get(nw, nb))), _bits(eo.fresh(layers, SEED, 0, 0)))
    b.close()                                                # ofx_destroy frees all of it


# ---------------------------------------------------------------- 9. the loop
LOOP = dict(N=8, M=3, P=4, W=48, H=40, T=10, lr=0.2, eval_arenas=2)       # tests/test_gpu_es.py's sizes
OPT = dict(optimizer="adam", weight_decay=0.005, sigma_init=0.05, sigma_lr=0.6)
LOOP_LAYERS = [8 + 2 * LOOP["W"] * LOOP["H"], 9, 4]


def _rollout(seed, init=True):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES, ESRollout
    L = LOOP
    b = ArenaBatch(L["N"], L["M"], width=L["W"], height=L["H"])
    es = ES(b, LOOP_LAYERS, seed, init=init, **OPT)
    roll = ESRollout(b, es, ["random"] * L["M"], seed, L["P"], None, L["lr"], ships=(0,), eval_arenas=L["eval_arenas"],
                     episode_ticks=L["T"], log_steps=True)
    return b, es, roll


class _HostBatch(eo.EvolutionOracleBatch):
    def state_dict(self):
        return {"episode": self.episode, "lockstep_count": self.lockstep_count}


def _run(roll, snap):
    T = LOOP["T"]
    snaps = [snap()]
    for _ in range(3):
        roll.run(T + (1 if len(snaps) == 1 else 0))          # up to and including the lock-step that ends a generation
        snaps.append(snap())
    return dict(fitness_log=list(roll.fitness_log), centre_log=list(roll.centre_log), weight_log=list(roll.weight_log),
                step_log=list(roll.step_log), snaps=snaps, generation=roll.generation, tick=roll.tick)


@pytest.fixture(scope="module")
def loop_run():
    b, es, roll = _rollout(sg.LOOP_SEED)
    out = _run(roll, lambda: _state(es))
    out["opt_steps"] = es.opt_steps
    b.close()
    return out


@pytest.fixture(scope="module")
def stand_in_run():
    from ofighters_amd.es import ESRollout
    L = LOOP
    b = _HostBatch(L["N"], L["M"], L["W"], L["H"])
    centre = sg.SigmaOracleES(b, LOOP_LAYERS, sg.LOOP_SEED, OPT["sigma_init"], sigma_lr=OPT["sigma_lr"], optimizer="adam",
                              weight_decay=0.005)
    roll = ESRollout(b, centre, ["random"] * L["M"], sg.LOOP_SEED, L["P"], None, L["lr"], ships=(0,),
                     eval_arenas=L["eval_arenas"], episode_ticks=L["T"], log_steps=True)
    return _run(roll, lambda: (centre.theta.copy(), centre.sigma_vec.copy(), centre.m.copy(), centre.v.copy()))


def test_adaptive_loop_equals_the_oracle_stand_in(loop_run, stand_in_run):
    dev, host, L = loop_run, stand_in_run, LOOP
    assert dev["generation"] == host["generation"] == 3 and dev["opt_steps"] == 3 and dev["tick"] == host["tick"]
    assert dev["fitness_log"] == host["fitness_log"] and dev["centre_log"] == host["centre_log"]
    assert len(dev["weight_log"]) == 3
    for gen, (x, y) in enumerate(zip(dev["weight_log"], host["weight_log"])):
        assert np.array_equal(_bits(x[0]), _bits(y[0])) and np.array_equal(_bits(x[1]), _bits(y[1])) and x[2] == y[2] == L["P"], gen
    assert dev["weight_log"][0][0].any(), "generation 0 of this seed has no untied pair: the first step saw no estimate"
    assert any(w[1].any() for w in dev["weight_log"]), "no generation had a pair off the baseline: sigma never stepped"
    for gen, (x, y) in enumerate(zip(dev["snaps"], host["snaps"])):
        _same(x, y, "after %d generations" % gen)
    assert dev["step_log"] == host["step_log"] and all(len(t) == 5 for t in dev["step_log"])
    # and each generation is the oracle's step from the previous state with the recorded weights
    for gen, (d, s, n_c) in enumerate(dev["weight_log"]):
        gscale, alpha, c1, k1, c2, k2, srate = sg.scalars("adam", L["lr"], n_c, gen + 1, 0.9, 0.999, OPT["sigma_lr"])
        old = dev["snaps"][gen]
        want = sg.step(old[0], old[1], old[2], old[3], d, s, sg.ADAM, gscale, 0.005, alpha, c1, k1, c2, k2, 1e-8, srate,
                       OPT["sigma_init"] / 64, OPT["sigma_init"] * 4, sg.LOOP_SEED, gen)
        _same(dev["snaps"][gen + 1], want[:4], "generation %d" % gen)
    sigma = dev["snaps"][3][1]
    assert np.unique(sigma).size > 1000, "sigma is still (nearly) uniform after three generations"
    print("weights per generation:", [(list(d), list(s), n) for d, s, n in dev["weight_log"]], "step_log:", dev["step_log"],
          "sigma min / mean / max: %.4g %.4g %.4g" % (sigma.min(), sigma.mean(), sigma.max()))


def test_adaptive_loop_resumes_bit_for_bit(loop_run, tmp_path):
    T = LOOP["T"]
    b, es, roll = _rollout(sg.LOOP_SEED)
    roll.run(T + 4)                                      # inside the second generation's episode
    path = es.save(str(tmp_path / "centre.npy"))
    state = roll.state_dict()
    assert state["generation"] == 1 and es.opt_steps == 1 and len(state["step_log"]) == 1 and len(state["weight_log"][0]) == 3
    _same(_state(es), loop_run["snaps"][1], "before the stop")
    b.close()
    b3, es3, roll3 = _rollout(sg.LOOP_SEED, init=False)  # fresh handles
    es3.load(path)
    assert es3.opt_steps == 1
    _same(_state(es3), loop_run["snaps"][1], "after ES.load")
    roll3.load_state_dict(state)
    roll3.run(loop_run["tick"] - (T + 4))
    assert roll3.generation == 3 and roll3.tick == loop_run["tick"] and es3.opt_steps == 3
    assert roll3.fitness_log == loop_run["fitness_log"] and roll3.centre_log == loop_run["centre_log"]
    assert roll3.step_log == loop_run["step_log"]
    _same(_state(es3), loop_run["snaps"][3], "the resumed run")
    for x, y in zip(roll3.weight_log, loop_run["weight_log"]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
    b3.close()
    # a scalar ES refuses the adaptive checkpoint, untouched
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ES
    b4 = ArenaBatch(1, 1, width=LOOP["W"], height=LOOP["H"])
    plain = ES(b4, LOOP_LAYERS, sg.LOOP_SEED, optimizer="adam", weight_decay=0.005)
    before = np.concatenate(b4.es_get(plain.n_weights, plain.n_biases))
    with pytest.raises(ValueError, match="sigma"):
        plain.load(path)
    assert np.array_equal(_bits(np.concatenate(b4.es_get(plain.n_weights, plain.n_biases))), _bits(before))
    b4.close()
