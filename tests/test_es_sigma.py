"""Per-element adaptive sigma of the ES centre, the CPU side: pair_utilities, the oracle's law against the older oracles
it must degenerate to, the scalars ES.update hands to the library, the refusals and the checkpoint of the Python layer on
a recording fake batch, the entry points in header / binding / library, and ESRollout's adaptive loop on the
oracle-backed stand-in of tests/test_es.py.  The kernels are held to the same oracle in tests/test_gpu_es_sigma.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from ofighters_amd import _native as nat
from ofighters_amd import engine, es
from ofighters_amd.es import pair_utilities
from tests import es_opt_oracle as oo
from tests import es_oracle as so
from tests import es_sigma_oracle as sg
from tests import evolution_oracle as eo
from tests.abi_header import ROOT, header_symbols
from tests.es_cases import bits as _bits
from tests.test_es_optimizer import _FakeBatch as _OptFakeBatch, _FakeBuffer

LAYERS = [8 + 2 * 48 * 40, 9, 4]
SEED = 0x0E512345
ELEMENTS = np.array([0, 1, 77, 3848 * 9 - 1, 3848 * 9, 34680], np.int64)   # both sides of the first layer's end


def test_entry_points_declared_bound_and_exported():
    declared, L = header_symbols(), C.CDLL(nat.LIB_PATH)
    names = ("create", "destroy", "get", "set", "member", "act", "step")
    for n in names:
        s = "ofx_es_sigma_" + n
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
        assert callable(getattr(engine.ArenaBatch, "es_sigma_" + n)), n
    assert nat.SIGNATURES["ofx_es_sigma_step"][1] == [C.c_void_p] * 3 + [C.c_int64, C.c_int32] + [C.c_double] * 11 + \
        [C.c_uint64, C.c_uint32, C.c_void_p]
    assert nat.SIGNATURES["ofx_es_sigma_act"][1][2:5] == [C.c_int64, C.c_uint64, C.c_uint32]
    header = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert "#define OFX_ES_RULE_PLAIN 0" in header
    assert (nat.ES_RULE_PLAIN, nat.ES_RULE_MOMENTUM, nat.ES_RULE_ADAM) == (sg.PLAIN, sg.MOMENTUM, sg.ADAM) == (0, 1, 2)
    assert sg.THIRD.hex() == "0x1.5555555555555p-2" and "0x1.5555555555555p-2" in header
    import ofighters_amd
    assert ofighters_amd.pair_utilities is pair_utilities


# ---------------------------------------------------------------- pair_utilities
def test_pair_utilities_hand_worked():
    # means 3, 1 | 2, 2 | 0, 5; slot 6 is the centre.  Ranks: member 4 -> 0, 1 -> 1, 2 and 3 -> 2.5, 0 -> 4, 5 -> 5
    s, c = np.array([6, 1, 4, 2, 0, 5, 99], np.int64), np.array([2, 1, 2, 1, 1, 1, 7], np.int32)
    d, w, n_c = pair_utilities(s, c)
    u = [r / 5 - 0.5 for r in (4, 1, 2.5, 2.5, 0, 5)]
    assert n_c == 6 and list(d) == [u[0] - u[1], 0.0, u[4] - u[5]]
    assert list(w) == [u[0] + u[1], u[2] + u[3], u[4] + u[5]]
    assert d[1] == 0.0 and w[1] == 0.0                      # a tied pair AT the baseline
    d2, w2, n2 = pair_utilities(s[:6], c[:6])               # without the centre's slot: the same
    assert np.array_equal(d, d2) and np.array_equal(w, w2) and n2 == 6
    # a tied pair ABOVE the baseline: d = 0, s != 0
    d, w, n_c = pair_utilities(np.array([5, 5, 1, 0]), np.array([1, 1, 1, 1]))
    assert n_c == 4 and d[0] == 0.0 and w[0] == 2 * (2.5 / 3 - 0.5) and w[1] == -w[0]
    # the best and the worst member in one pair: d = 1, s = 0 exactly (u = +0.5 and -0.5); the inner pair's two u are
    # rounded quotients and their sum is what float64 makes of it, not 0
    d, w, n_c = pair_utilities(np.array([9, 0, 4, 3]), np.array([1, 1, 1, 1]))
    assert list(d) == [1.0, (2 / 3 - 0.5) - (1 / 3 - 0.5)] and list(w) == [0.0, (2 / 3 - 0.5) + (1 / 3 - 0.5)]


def test_pair_utilities_properties_and_the_oracle():
    rs = np.random.RandomState(4)
    seen_tie = seen_incomplete = 0
    for _ in range(80):
        n_pairs = int(rs.randint(1, 9))
        s = rs.randint(-6, 7, 2 * n_pairs + 1).astype(np.int64)
        c = rs.randint(0, 3, 2 * n_pairs + 1).astype(np.int32)
        d, w, n_c = pair_utilities(s, c)
        want_d, want_w, want_n = sg.pair_utilities(s, c)
        assert n_c == want_n and np.array_equal(_bits(d), _bits(want_d)) and np.array_equal(_bits(w), _bits(want_w))
        pd, pn = es.pair_weights(s, c)
        assert pn == n_c and np.array_equal(_bits(d), _bits(pd)), "d is pair_weights' to the bit"
        d0, w0, n0 = pair_utilities(s[:-1], c[:-1])          # the trailing centre slot is ignored
        assert n0 == n_c and np.array_equal(_bits(d0), _bits(d)) and np.array_equal(_bits(w0), _bits(w))
        complete = (c[:-1].reshape(-1, 2) > 0).all(axis=1)
        assert not w[~complete].any() and not d[~complete].any() and (np.abs(w) <= 1.0).all()
        seen_incomplete += int((~complete).any())
        mean = s[:-1].reshape(-1, 2)[complete] / c[:-1].reshape(-1, 2)[complete]
        seen_tie += int((mean[:, 0] == mean[:, 1]).any())
        # swapping every pair's two members leaves s and negates d, exactly
        swap = np.arange(2 * n_pairs).reshape(-1, 2)[:, ::-1].ravel()
        d2, w2, n2 = pair_utilities(s[:-1][swap], c[:-1][swap])
        assert n2 == n_c and np.array_equal(_bits(w2), _bits(w)) and np.array_equal(d2, -d)
        # the centred ranks sum to 0, so do the pair utilities: each u is a multiple of 0.5 / (n_c - 1) rounded once
        assert abs(w.sum()) <= 1e-12 * max(n_c, 1)
    assert seen_tie > 10 and seen_incomplete > 10
    # all means equal, a single tied pair, nobody flown, too few flown: all zeros
    for s, c, n in (([4, 2, 2, 6], [2, 1, 1, 3], 4), ([3, 3, 1, 0], [1, 1, 1, 0], 2), ([0, 0, 0, 0], [0, 0, 0, 0], 0),
                    ([5, 1, 0, 0], [1, 0, 0, 1], 0)):
        d, w, n_c = pair_utilities(np.array(s, np.int64), np.array(c, np.int32))
        assert n_c == n and not d.any() and not w.any()
        assert [x.tolist() for x in sg.pair_utilities(s, c)[:2]] == [d.tolist(), w.tolist()]
    with pytest.raises(ValueError):
        pair_utilities(np.zeros(1, np.int64), np.zeros(1, np.int32))
    with pytest.raises(ValueError):
        pair_utilities(np.zeros(4, np.int64), np.zeros(5, np.int32))


def test_pair_weights_is_pair_utilities_on_every_bit():
    """pair_weights(s, c) == (pair_utilities(s, c)[0], [2]) - one ranking behind both - at P = 2, 4, 6 with and without
    the centre's slot: ties, an incomplete pair, all means equal, fewer than two flown members."""
    cases = {2: [([3, 1], [1, 1]), ([2, 2], [1, 1]), ([3, 1], [1, 0]), ([0, 0], [0, 0])],
             4: [([6, 1, 4, 2], [2, 1, 2, 1]), ([5, 5, 1, 0], [1, 1, 1, 1]), ([9, 0, 4, 3], [1, 1, 0, 1]),
                 ([4, 2, 2, 6], [2, 1, 1, 3]), ([5, 1, 0, 0], [1, 0, 0, 1])],
             6: [([6, 1, 4, 2, 0, 5], [2, 1, 2, 1, 1, 1]), ([1, 1, 1, 2, 2, 2], [1, 1, 1, 1, 1, 1]),
                 ([7, -3, 4, 4, 0, 5], [1, 1, 1, 1, 0, 2]), ([3, 3, 6, 6, 9, 9], [1, 1, 2, 2, 3, 3]),
                 ([5, 1, 0, 0, 2, 2], [1, 0, 0, 1, 0, 0])]}
    for P, rows in cases.items():
        for s, c in rows:
            for extra in ((), (99,)):                          # [P], then [P + 1] with the centre flown
                sv, cv = np.array(list(s) + list(extra), np.int64), np.array(list(c) + [7] * len(extra), np.int32)
                assert sv.shape == (P + len(extra),)
                d, n_c = es.pair_weights(sv, cv)
                ud, uw, un = pair_utilities(sv, cv)
                assert n_c == un and type(n_c) is type(un), (s, c)
                assert d.dtype == ud.dtype == np.float64 and d.shape == ud.shape == (P // 2,)
                assert np.array_equal(_bits(d), _bits(ud)), (s, c)


# ---------------------------------------------------------------- the oracle against the oracles it degenerates to
def _state(n, seed=5):
    rs = np.random.RandomState(seed)
    theta = rs.uniform(0.25, 1.0, n) * rs.choice([-1.0, 1.0], n)
    return theta, rs.uniform(-0.1, 0.1, n), rs.uniform(0, 0.01, n)


ADAM_SC = dict(gscale=1.0 / 8, decay=0.005, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8)
D, S, GEN = np.array([0.4, 0.0, -1.0, 0.25, 0.0]), np.array([0.3, 0.5, 0.0, -0.8, 0.0]), 3   # every zero / nonzero mix


def test_uniform_sigma_gives_the_scalar_member():
    theta = eo.fresh(LAYERS, SEED, 0, 0)
    for sigma in (0.05, 0.07, 1.0):
        vec = np.full(theta.shape, sigma)
        for m in range(7):
            assert np.array_equal(_bits(sg.member(theta, vec, SEED, m, 6, GEN)), _bits(so.member(theta, SEED, m, 6, sigma, GEN)))
    # and a vector that is not uniform moves exactly the elements whose width differs
    vec = np.full(theta.shape, 0.05)
    vec[::3] = 0.2
    got, base = sg.member(theta, vec, SEED, 1, 6, GEN), so.member(theta, SEED, 1, 6, 0.05, GEN)
    assert np.array_equal(_bits(got[1::3]), _bits(base[1::3])) and (got[::3] != base[::3]).mean() > 0.99
    pick = np.array([0, 5, 3848 * 9 - 1, 3848 * 9, theta.size - 1])
    assert np.array_equal(sg.member(theta[pick], vec[pick], SEED, 3, 6, GEN, elements=pick), sg.member(theta, vec, SEED, 3, 6, GEN)[pick])


@pytest.mark.parametrize("rule", [sg.PLAIN, sg.MOMENTUM, sg.ADAM])
def test_zero_utilities_leave_sigma(rule):
    """s = 0: qs is a sum of +-0 from +0.0, so r = srate * 0 = +-0, f = 1 and sn = sigma * 1 = sigma, whatever srate."""
    theta, m, v = _state(6)
    sigma = np.array([0.05, 0.01, 0.2, 0.05, 5e-324, 0.07])
    for srate in (0.0, 0.3, -7.5, 1e300):
        out = sg.step(theta, sigma, m, v, D, np.zeros(5), rule, srate=srate, smin=5e-324, smax=0.2, seed=SEED,
                      generation=GEN, elements=ELEMENTS, **ADAM_SC)
        assert np.array_equal(_bits(out[1]), _bits(sigma)) and not out[6].any()
        assert (out[0] != theta).all()


@pytest.mark.parametrize("rule", [sg.MOMENTUM, sg.ADAM])
@pytest.mark.parametrize("decay", [0.0, 0.005])
def test_unit_sigma_and_zero_rate_give_the_optimiser_step(rule, decay):
    """sigma = 1: sg = 1 * g = g.  srate = 0: r = +-0, f = 1, sigma' = 1.  The pairs listed for their s alone add +-0 to
    g.  So theta', m', v' are tests/es_opt_oracle.py's, bit for bit."""
    theta, m, v = _state(6)
    sc = dict(ADAM_SC, decay=decay)
    out = sg.step(theta, np.ones(6), m, v, D, S, rule, srate=0.0, smin=0.5, smax=2.0, seed=SEED, generation=GEN,
                  elements=ELEMENTS, **sc)
    want = oo.step(theta, m, v, D, rule, seed=SEED, generation=GEN, elements=ELEMENTS, **sc)
    for got, w, name in zip((out[0], out[2], out[3], out[4], out[5]), want, ("theta", "m", "v", "q", "step")):
        assert np.array_equal(_bits(got), _bits(w)), name
    assert np.array_equal(_bits(out[1]), _bits(np.ones(6))) and not out[6].any()


def test_plain_rule_against_the_bare_update():
    """PLAIN, decay = 0, sigma = 1: step = alpha * (gscale * g); ofx_es_update's is (alpha * gscale) * g.
    With alpha a power of two both round once, at the same place: EQUAL bits.  Otherwise each step carries two
    roundings, so the two differ by at most 4 * 2^-53 |step|; here |theta| >= 0.25 and |step| < 0.04 (|g| < 2 * 1.65,
    alpha <= 0.07, gscale = 1 / 6), so that is under 2^-53 |theta'| < 1 ulp of theta', the two exact sums enclose at
    most one rounding boundary and the results differ by AT MOST 1 ULP - and some do differ, which is why this is not
    an equality."""
    n = 4096
    theta, m, v = _state(n, 9)
    elements = np.arange(n, dtype=np.int64)
    worst = 0
    for alpha, exact in ((0.25, True), (0.03, False), (0.07, False)):
        out = sg.step(theta, np.ones(n), m, v, D, S, sg.PLAIN, 1.0 / 6, 0.0, alpha, 0.0, 1.0, 0.0, 1.0, 1e-8, 0.0, 0.5, 2.0,
                      SEED, GEN, elements)
        want = so.update(theta, D, alpha * (1.0 / 6), SEED, GEN, elements=elements)
        assert exact or (np.abs(out[5]).max() < 0.04 and np.abs(theta).min() >= 0.25)
        diff = np.abs(_bits(out[0]).astype(np.int64) - _bits(want).astype(np.int64))
        assert np.array_equal(np.sign(out[0]), np.sign(want))
        if exact:
            assert not diff.any(), "a power-of-two alpha: equal bits"
        else:
            assert diff.max() <= 1
            worst = max(worst, int(diff.max()))
        assert np.array_equal(_bits(out[2]), _bits(m)) and np.array_equal(_bits(out[3]), _bits(v)), "PLAIN touched a moment"
    assert worst == 1, "the two orders of multiplication never differed: state the equality instead"


def test_law_against_a_scalar_restatement_and_the_clamps():
    theta, m, v = _state(6)
    sigma = np.array([0.05, 0.01, 0.2, 0.05, 0.03, 0.07])
    srate, smin, smax = 0.9, 0.03, 0.06
    out = sg.step(theta, sigma, m, v, D, S, sg.ADAM, srate=srate, smin=smin, smax=smax, seed=SEED, generation=GEN,
                  elements=ELEMENTS, **ADAM_SC)
    for j, e in enumerate(ELEMENTS):
        g = qs = 0.0
        for i, (di, si) in enumerate(zip(D, S)):
            x = so.eps_scalar(SEED, i, e, GEN)
            t = float(di) * x
            g = g + t
            xx = x * x
            c = xx - sg.THIRD
            u = float(si) * c
            qs = qs + u                                      # every pair, the unlisted ones too: +-0 changes nothing
        sgg = float(sigma[j]) * g
        want = oo.step_scalar(float(theta[j]), float(m[j]), float(v[j]), sgg, oo.ADAM, **ADAM_SC)
        r = srate * qs
        f = 1.0 + r
        sn = float(sigma[j]) * f
        clamped = sn < smin or sn > smax
        sn = min(max(sn, smin), smax)
        for got, w, name in zip((out[0][j], out[2][j], out[3][j], out[1][j]), want + (sn,), ("theta", "m", "v", "sigma")):
            assert _bits(got) == _bits(w), "element %d %s: %r != %r" % (e, name, got, w)
        assert out[6][j] == float(clamped)
    assert out[1][1] == smin and out[1][2] == smax and out[6][1] == out[6][2] == 1.0


def test_fixed_order_sum_is_a_sum_in_storage_order():
    layers = [104, 9, 4]
    G = eo.n_elements(layers)
    perm = sg.storage_order(layers)
    assert sorted(perm) == list(range(G)) and perm[1] == 104 and perm[9] == 1 and perm[104 * 9] == 104 * 9
    x = np.random.RandomState(2).uniform(0, 1, G)
    got = sg.fixed_order_sum(x, layers)
    assert abs(got - math.fsum(x)) <= (G - 1) * 2.0 ** -53 * math.fsum(x)
    assert sg.fixed_order_sum(np.ones(G), layers) == float(G)
    # the order matters and is the stated one: 256 ones, then a 2^53 that absorbs every later one
    big = [8 + 2 * 48 * 40, 9, 4]
    y = np.zeros(eo.n_elements(big))
    y[sg.storage_order(big)[:256]] = 1.0
    y[sg.storage_order(big)[256]] = 2.0 ** 53
    y[sg.storage_order(big)[257:260]] = 1.0
    # workgroup 1's tree: (2^53 + 0) ... the three ones meet each other before they meet 2^53: 1 + 1 = 2 survives
    assert sg.fixed_order_sum(y, big) == 256.0 + 2.0 ** 53 + 2.0


# ---------------------------------------------------------------- the Python layer on a recording fake batch
class _FakeBatch(_OptFakeBatch):
    def __init__(self, n_weights, n_biases):
        super().__init__(n_weights, n_biases)
        self.sigma = None

    def es_sigma_create(self, sigma0):
        self.calls.append(("es_sigma_create", sigma0))
        self.sigma = np.full_like(self.theta, sigma0)

    def es_sigma_get(self, nw, nb):
        return self._split(self.sigma)

    def es_sigma_set(self, w, b):
        self.calls.append(("es_sigma_set",))
        self.sigma = np.concatenate([w, b])

    def es_sigma_member(self, *a):
        self.calls.append(("es_sigma_member",) + a)
        return self._split(self.theta)

    def es_member(self, *a):
        self.calls.append(("es_member",) + a)
        return self._split(self.theta)

    def es_sigma_act(self, *a, **kw):
        self.calls.append(("es_sigma_act",) + a)

    def es_act(self, *a, **kw):
        self.calls.append(("es_act",) + a)

    def es_sigma_step(self, d, s, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate, smin, smax, seed, generation,
                      stats_ptr=None):
        self.calls.append(("es_sigma_step", np.array(d), np.array(s), rule, gscale, decay, alpha, c1, k1, c2, k2, eps, srate,
                           smin, smax, seed, generation, stats_ptr))


SMALL = [104, 9, 4]


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(engine, "DeviceBuffer", _FakeBuffer)
    return _FakeBatch(*es.genome_sizes(SMALL))


@pytest.mark.parametrize("optimizer,rule", [(None, 0), ("momentum", 1), ("adam", 2)])
def test_adaptive_calls_and_scalars(fake, optimizer, rule):
    beta1, beta2, eps, wd = 0.8, 0.99, 1e-6, 0.005
    centre = es.ES(fake, SMALL, 7, optimizer=optimizer, beta1=beta1, beta2=beta2, adam_eps=eps, weight_decay=wd,
                   sigma_init=0.08, sigma_lr=0.6)
    assert [c[0] for c in fake.calls] == ["es_create"] + (["es_opt_create"] if optimizer else []) + ["es_sigma_create", "es_init"]
    assert centre.adaptive and (centre.sigma_min, centre.sigma_max) == (0.08 / 64, 0.08 * 4)
    assert centre._stats.nbytes == 40
    d, s, lr, n_c = np.array([0.5, 0.0, -1.0]), np.array([0.0, 0.25, -0.5]), 0.07, 6
    for t in (1, 2, 3):
        centre.update(d, lr, None, n_c, generation=10 + t, s=s)
        assert centre.opt_steps == (t if optimizer else 0)
        (name, got_d, got_s, got_rule, gscale, decay, alpha, c1, k1, c2, k2, got_eps, srate, smin, smax, seed, generation,
         stats_ptr) = fake.calls[-1]
        assert name == "es_sigma_step" and np.array_equal(got_d, d) and np.array_equal(got_s, s) and got_rule == rule
        assert (seed, generation) == (7, 10 + t) and stats_ptr == centre._stats.ptr
        assert gscale == 1.0 / n_c and srate == 0.6 / n_c and decay == wd and got_eps == eps
        assert (smin, smax) == (0.08 / 64, 0.08 * 4)
        if optimizer is None:
            assert (alpha, c1, k1, c2, k2) == (lr, 0.0, 1.0, 0.0, 1.0)
        else:
            assert (c1, k1, c2, k2) == (beta1, 1.0 - beta1, beta2, 1.0 - beta2)
            assert alpha == (lr if optimizer == "momentum" else lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t))
        assert (gscale, alpha, c1, k1, c2, k2, srate) == sg.scalars(optimizer, lr, n_c, t, beta1, beta2, 0.6)
    n = len(fake.calls)
    # nothing is silently ignored: a number for sigma, a missing s
    for call, word in ((lambda: centre.update(d, lr, 0.05, n_c, 0, s=s), "sigma"), (lambda: centre.update(d, lr, None, n_c, 0), "s is"),
                       (lambda: centre.act(0.05, 0), "sigma"), (lambda: centre.member(0, 4, 0.05, 0), "sigma"),
                       (lambda: centre.update(d, lr, None, n_c, 0, s=s[:2]), "s is"),
                       (lambda: centre.update(d, lr, None, n_c, 0, s=np.array([0.0, np.nan, 0.0])), "s is"),
                       (lambda: centre.update(d, lr, None, 1, 0, s=s), "n_c")):
        with pytest.raises(ValueError, match=word):
            call()
    assert len(fake.calls) == n and centre.opt_steps == (3 if optimizer else 0)
    centre.assign(np.zeros((2, 2), np.int32), 4)
    centre.act(None, 3)
    assert fake.calls[-1][0] == "es_sigma_act" and fake.calls[-1][2:] == (4, 7, 3)
    centre.member(1, 4, None, 3)
    assert fake.calls[-1][:5] == ("es_sigma_member", 1, 4, 7, 3)
    centre._stats.host = np.array([4.0, 0.25, 9.0, 1.5, 2.0])
    assert centre.step_stats() == (4.0, 0.25, 9.0, 1.5, 2.0) and fake.calls[-1] == ("sync",)
    W, B = centre.sigmas()
    assert [x.shape for x in W] == [(9, 104), (4, 9)] and [x.shape for x in B] == [x.shape for x in centre.centre()[1]]
    centre.set_sigmas([2 * x for x in W], [2 * x for x in B])
    assert fake.calls[-1] == ("es_sigma_set",) and np.array_equal(fake.sigma, np.full(fake.theta.shape, 0.16))


def test_a_scalar_es_is_todays_and_refuses_the_adaptive_calls(fake):
    centre = es.ES(fake, SMALL, 7)
    assert [c[0] for c in fake.calls] == ["es_create", "es_init"] and centre.adaptive is False
    d = np.array([0.5, -1.0])
    centre.update(d, 0.1, 0.05, 4, 2)
    assert fake.calls[-1][0] == "es_update" and fake.calls[-1][2] == 0.1 / (4 * 0.05)
    n = len(fake.calls)
    for call, word in ((lambda: centre.update(d, 0.1, None, 4, 2), "sigma"), (lambda: centre.update(d, 0.1, 0.05, 4, 2, s=d), "s must"),
                       (lambda: centre.act(None, 0), "sigma"), (lambda: centre.member(0, 4, None, 0), "sigma"),
                       (centre.sigmas, "sigma_init"), (lambda: centre.set_sigmas(None, None), "sigma_init")):
        with pytest.raises(ValueError, match=word):
            call()
    assert len(fake.calls) == n


def test_constructor_refuses_before_the_library_is_touched(fake):
    nan, inf = float("nan"), float("inf")
    bad = [("sigma_init", dict(sigma_init=0.0)), ("sigma_init", dict(sigma_init=-0.05)), ("sigma_init", dict(sigma_init=nan)),
           ("sigma_init", dict(sigma_init=inf)), ("sigma_lr", dict(sigma_init=0.05, sigma_lr=-0.1)),
           ("sigma_lr", dict(sigma_init=0.05, sigma_lr=nan)), ("sigma_lr", dict(sigma_init=0.05, sigma_lr=inf)),
           ("sigma_min", dict(sigma_init=0.05, sigma_min=0.0)), ("sigma_min", dict(sigma_init=0.05, sigma_min=-1.0)),
           ("sigma_min", dict(sigma_init=0.05, sigma_min=nan)), ("sigma_max", dict(sigma_init=0.05, sigma_max=inf)),
           ("sigma_max", dict(sigma_init=0.05, sigma_min=0.04, sigma_max=0.03)),
           ("sigma_init", dict(sigma_init=0.05, sigma_min=0.06)), ("sigma_init", dict(sigma_init=0.05, sigma_max=0.04)),
           ("sigma_init", dict(sigma_min=0.01)), ("sigma_init", dict(sigma_max=0.1)),
           ("weight_decay", dict(weight_decay=0.005)), ("optimizer", dict(sigma_init=0.05, optimizer="sgd"))]
    for word, kw in bad:
        with pytest.raises(ValueError, match=word):
            es.ES(fake, SMALL, 7, **kw)
    assert fake.calls == []
    es.ES(fake, SMALL, 7, sigma_init=0.05, weight_decay=0.005)          # the PLAIN rule has a decay term
    es.ES(_FakeBatch(*es.genome_sizes(SMALL)), SMALL, 7, sigma_init=0.05, sigma_lr=0.0, sigma_min=0.05, sigma_max=0.05)


def test_check_es_sigma_meta_names_each_field():
    want = es.es_sigma_meta(0.2, 0.001, 0.2)
    assert want == {"lr": 0.2, "min": 0.001, "max": 0.2}
    G = 17
    meta = {"layers": [1], "seed": 2, "sigma": dict(want)}
    es.check_es_sigma_meta(meta, want)
    es.check_es_sigma_meta(meta, want, (G,), np.float64, G)
    es.check_es_sigma_meta({"layers": [1], "seed": 2}, None)
    for field, other in (("lr", 0.6), ("min", 0.002), ("max", 0.1)):
        with pytest.raises(ValueError, match="sigma %s" % field):
            es.check_es_sigma_meta(dict(meta, sigma=dict(want, **{field: other})), want)
        with pytest.raises(ValueError, match="no field '%s'" % field):
            es.check_es_sigma_meta(dict(meta, sigma={k: v for k, v in want.items() if k != field}), want)
    with pytest.raises(ValueError, match="no sigma block"):
        es.check_es_sigma_meta({"layers": [1], "seed": 2}, want)
    with pytest.raises(ValueError, match="has a sigma block"):
        es.check_es_sigma_meta(meta, None)
    with pytest.raises(ValueError, match="shape"):
        es.check_es_sigma_meta(meta, want, (G + 1,), np.float64, G)
    with pytest.raises(ValueError, match="shape"):
        es.check_es_sigma_meta(meta, want, (1, G), np.float64, G)
    with pytest.raises(ValueError, match="dtype"):
        es.check_es_sigma_meta(meta, want, (G,), np.float32, G)


def test_checkpoint_carries_sigma_and_refuses_untouched(fake, tmp_path):
    nw, nb = es.genome_sizes(SMALL)
    G = nw + nb
    kw = dict(optimizer="adam", weight_decay=0.005, sigma_init=0.05, sigma_lr=0.6)
    a = es.ES(fake, SMALL, 7, **kw)
    rs = np.random.RandomState(1)
    fake.theta, fake.m, fake.v, fake.sigma = rs.uniform(-1, 1, G), rs.uniform(-1, 1, G), rs.uniform(0, 1, G), rs.uniform(0.01, 0.2, G)
    a.opt_steps = 5
    path = a.save(str(tmp_path / "centre.npy"))
    sig = np.load(path + ".sigma.npy")
    assert sig.dtype == np.float64 and sig.shape == (G,) and np.array_equal(_bits(sig), _bits(fake.sigma))
    meta = json.load(open(path + ".json"))
    assert meta["sigma"] == {"lr": 0.6, "min": 0.05 / 64, "max": 0.05 * 4} and meta["optimizer"]["steps"] == 5
    assert sorted(meta) == ["layers", "optimizer", "seed", "sigma"]

    def fresh(**kw2):
        other = _FakeBatch(nw, nb)
        return other, es.ES(other, SMALL, 7, **kw2)

    b2, same = fresh(**kw)
    same.load(path)
    assert same.opt_steps == 5 and np.array_equal(_bits(b2.theta), _bits(fake.theta))
    assert np.array_equal(_bits(b2.sigma), _bits(fake.sigma)) and np.array_equal(_bits(b2.m), _bits(fake.m))

    def refused(word, path, **kw2):
        b3, other = fresh(**kw2)
        n, before = len(b3.calls), (b3.theta.copy(), b3.sigma.copy() if b3.sigma is not None else None)
        with pytest.raises(ValueError, match=word):
            other.load(path)
        assert len(b3.calls) == n and other.opt_steps == 0 and np.array_equal(b3.theta, before[0]), word
        assert before[1] is None or np.array_equal(b3.sigma, before[1])

    refused("has a sigma block", path, optimizer="adam", weight_decay=0.005)        # unwanted
    refused("sigma lr", path, **dict(kw, sigma_lr=0.2))                             # differs
    refused("sigma min", path, **dict(kw, sigma_min=0.01))
    refused("sigma max", path, **dict(kw, sigma_max=0.1))
    refused("has an optimizer block", path, sigma_init=0.05, sigma_lr=0.6)
    # the array's shape, dtype and values
    for word, arr in (("shape", sig[:-1]), ("shape", sig.reshape(1, G)), ("dtype", sig.astype(np.float32)),
                      ("not finite and > 0", np.where(np.arange(G) == 3, 0.0, sig)),
                      ("not finite and > 0", np.where(np.arange(G) == 3, np.nan, sig))):
        np.save(open(path + ".sigma.npy", "wb"), arr)
        refused(word, path, **kw)
    np.save(open(path + ".sigma.npy", "wb"), sig)
    # missing: a non-adaptive checkpoint is byte for byte today's, and an adaptive ES refuses it
    b4, plain = fresh()
    plain_path = plain.save(str(tmp_path / "plain.npy"))
    assert json.load(open(plain_path + ".json")) == {"layers": SMALL, "seed": 7}
    assert not (tmp_path / "plain.npy.sigma.npy").exists() and not (tmp_path / "plain.npy.opt.npy").exists()
    refused("no sigma block", plain_path, sigma_init=0.05)
    # PLAIN adaptive: no moments file, the sigma block alone
    b5, pl = fresh(sigma_init=0.05)
    p5 = pl.save(str(tmp_path / "pl.npy"))
    assert sorted(json.load(open(p5 + ".json"))) == ["layers", "seed", "sigma"] and not (tmp_path / "pl.npy.opt.npy").exists()
    b6, pl2 = fresh(sigma_init=0.05)
    b6.sigma[:] = 0.01
    pl2.load(p5)
    assert np.array_equal(b6.sigma, np.full(G, 0.05))


# ---------------------------------------------------------------- the loop on the stand-in of tests/test_es.py
class _Batch(eo.EvolutionOracleBatch):
    def state_dict(self):
        return {"episode": self.episode, "lockstep_count": self.lockstep_count}

    def load_state_dict(self, d):
        self.episode, self.lockstep_count = d["episode"], d["lockstep_count"]


N, M, P, TICKS, LR = 4, 3, 4, 6, 0.1


def _stand_in(optimizer="adam", log_steps=True):
    b = _Batch(N, M, 48, 40)
    centre = sg.SigmaOracleES(b, LAYERS, SEED, 0.05, sigma_lr=0.6, optimizer=optimizer, weight_decay=0.005)
    roll = es.ESRollout(b, centre, ["random"] * M, SEED, P, None, LR, ships=(0, 2), eval_arenas=1, episode_ticks=TICKS,
                        log_steps=log_steps)
    return b, centre, roll


def test_adaptive_rollout_on_the_stand_in():
    b, centre, roll = _stand_in()
    roll.run(2 * TICKS + 2)                                  # inside the third generation's episode
    assert roll.adaptive and roll.sigma is None and roll.generation == 2
    kinds = [c[0] for c in centre.calls]
    acts = [c for c in centre.calls if c[0] == "act"]
    assert [c[1] for c in acts] == list(range(2 * TICKS + 2)) and all(c[2] is None for c in acts)
    i = kinds.index("fitness")
    assert kinds[i:i + 5] == ["fitness", "update", "step_stats", "assign", "act"]
    stepped = [g for g, w in enumerate(roll.weight_log) if w[2] >= 2]
    assert stepped and stepped[0] == 0 and len(roll.step_log) == len(stepped) == centre.opt_steps
    updates = [c for c in centre.calls if c[0] == "update"]
    assert [c[1] for c in updates] == stepped
    for t, c in enumerate(updates, 1):
        d, s, n_c = roll.weight_log[c[1]]
        assert np.array_equal(c[2], d) and np.array_equal(c[3], s), "d and s of pair_utilities reach update"
        assert c[4] == sg.scalars("adam", LR, n_c, t, 0.9, 0.999, 0.6)
    for d, s, n_c in roll.weight_log:
        assert d.shape == s.shape == (P // 2,) and isinstance(n_c, int)
    assert any(w[1].any() for w in roll.weight_log), "no generation had a pair off the baseline"
    for entry in roll.step_log:
        assert len(entry) == 5 and all(isinstance(x, float) for x in entry) and all(x > 0 for x in entry[:4])
    assert roll.step_log[-1] == centre.last
    assert np.unique(centre.sigma_vec).size > 1, "sigma is still uniform after two adaptive steps"
    # state_dict round trip: s travels in weight_log
    state = roll.state_dict()
    assert all(len(w) == 3 for w in state["weight_log"]) and state["step_log"] == roll.step_log
    b2, centre2, roll2 = _stand_in()
    centre2.theta, centre2.sigma_vec = centre.theta.copy(), centre.sigma_vec.copy()
    centre2.m, centre2.v, centre2.opt_steps = centre.m.copy(), centre.v.copy(), centre.opt_steps
    roll2.load_state_dict(state)
    d2 = roll2.state_dict()
    assert sorted(d2) == sorted(state) and roll2.generation == 2 and roll2.step_log == roll.step_log
    for u, w in zip(state["weight_log"], d2["weight_log"]):
        assert np.array_equal(u[0], w[0]) and np.array_equal(u[1], w[1]) and u[2] == w[2]
    assert np.array_equal(centre2.member_of, centre.member_of)


def test_rollout_sigma_is_none_exactly_when_adaptive():
    b = _Batch(2, 2, 48, 40)
    adaptive = sg.SigmaOracleES(b, LAYERS, SEED, 0.05)
    scalar = so.OracleES(b, LAYERS, SEED)
    with pytest.raises(ValueError, match="sigma must be None"):
        es.ESRollout(b, adaptive, ["random"] * 2, SEED, 4, 0.05, 0.1)
    with pytest.raises(ValueError, match="sigma must be a number"):
        es.ESRollout(b, scalar, ["random"] * 2, SEED, 4, None, 0.1)
    es.ESRollout(b, adaptive, ["random"] * 2, SEED, 4, None, 0.1)
    roll = es.ESRollout(b, scalar, ["random"] * 2, SEED, 4, 0.05, 0.1)
    assert roll.adaptive is False and roll.sigma == 0.05
    # PLAIN adaptive through the loop: steps without an optimiser, opt_steps stays 0
    b2, centre, roll2 = _stand_in(optimizer=None, log_steps=False)
    roll2.run(TICKS + 1)
    assert centre.opt_steps == 0 and [c[0] for c in centre.calls].count("update") == 1 and roll2.step_log == []
    assert centre.calls[[c[0] for c in centre.calls].index("update")][4][1:6] == (LR, 0.0, 1.0, 0.0, 1.0)
