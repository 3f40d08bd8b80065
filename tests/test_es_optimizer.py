"""The optimiser of the ES centre, the CPU side: the oracle's law against a scalar restatement, the step scale that
follows from it, the scalars ES.update hands to the library, the refusals and the checkpoint of the Python layer on a
recording fake batch, the entry points in header / binding / library, and ESRollout's step log on the oracle-backed
stand-in of tests/test_es.py.  The kernel is held to the same oracle in tests/test_gpu_es_optimizer.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from ofighters_amd import _native as nat
from ofighters_amd import engine, es
from tests import es_opt_oracle as oo
from tests import es_oracle as so
from tests import evolution_oracle as eo
from tests.abi_header import ROOT, header_symbols
from tests.es_cases import bits as _bits

LAYERS = [8 + 2 * 48 * 40, 9, 4]
SEED = 0x0E512345


def test_entry_points_declared_bound_and_exported():
    declared, L = header_symbols(), C.CDLL(nat.LIB_PATH)
    for s in ("ofx_es_opt_create", "ofx_es_opt_destroy", "ofx_es_opt_get", "ofx_es_opt_set", "ofx_es_step"):
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    assert nat.SIGNATURES["ofx_es_step"][1][2:] == [C.c_int64, C.c_int32] + [C.c_double] * 8 + \
        [C.c_uint64, C.c_uint32, C.c_void_p]
    header = open(os.path.join(ROOT, "include", "ofx.h")).read()
    assert "#define OFX_ES_RULE_MOMENTUM 1" in header and "#define OFX_ES_RULE_ADAM 2" in header
    assert (nat.ES_RULE_MOMENTUM, nat.ES_RULE_ADAM) == (oo.MOMENTUM, oo.ADAM) == (1, 2)
    for name in ("es_opt_create", "es_opt_destroy", "es_opt_get", "es_opt_set", "es_step"):
        assert callable(getattr(engine.ArenaBatch, name)), name


# ---------------------------------------------------------------- the law
@pytest.mark.parametrize("rule", [oo.MOMENTUM, oo.ADAM])
@pytest.mark.parametrize("decay", [0.0, 0.005])
def test_oracle_law_equals_the_scalar_restatement(rule, decay):
    """The vector oracle against one Python-float operation per line with math.sqrt, on a few elements that straddle
    the first layer's end, with nonzero moments and a zero weight among the pairs."""
    elements = np.array([0, 1, 77, 3848 * 9 - 1, 3848 * 9, 34680], np.int64)
    rs = np.random.RandomState(5)
    theta, m, v = rs.uniform(-1, 1, 6), rs.uniform(-0.1, 0.1, 6), rs.uniform(0, 0.01, 6)
    theta[1], m[2], v[3] = -0.0, 0.0, 0.0
    d, generation = np.array([0.4, 0.0, -1.0, 0.25]), 3
    sc = dict(gscale=1.0 / (8 * 0.05), decay=decay, alpha=0.03, c1=0.9, k1=1.0 - 0.9, c2=0.999, k2=1.0 - 0.999, eps=1e-8)
    t2, m2, v2, q, st = oo.step(theta, m, v, d, rule, seed=SEED, generation=generation, elements=elements, **sc)
    for j, e in enumerate(elements):
        G = 0.0
        for i, di in enumerate(d):
            if di != 0.0:
                t = float(di) * so.eps_scalar(SEED, i, e, generation)
                G = G + t
        want = oo.step_scalar(float(theta[j]), float(m[j]), float(v[j]), G, rule, **sc)
        for got, w, name in zip((t2[j], m2[j], v2[j]), want, ("theta", "m", "v")):
            assert _bits(got) == _bits(w), "element %d %s: %r != %r" % (e, name, got, w)
    assert (t2 != theta).all() and (m2 != m).all()
    if rule == oo.MOMENTUM:
        assert np.array_equal(_bits(v2), _bits(v)), "momentum touched v"
    else:
        assert (v2 != v).all()
    # the zero weight is left out or added: the same bits (a sum that starts at +0.0 is never -0.0)
    g_all = np.zeros(6)
    for i, di in enumerate(d):
        g_all = g_all + np.multiply(di, so.eps(SEED, i, elements, generation))
    assert np.array_equal(_bits(g_all), _bits(oo.estimate((6,), d, SEED, generation, elements)))


def test_all_zero_weights_still_decay():
    """d = 0 everywhere: q = -decay * theta, so theta moves under decay and m decays towards it."""
    theta, m, v = np.array([0.5, -0.25]), np.array([0.1, 0.1]), np.zeros(2)
    t2, m2, v2, q, st = oo.step(theta, m, v, np.zeros(3), oo.MOMENTUM, 2.5, 0.005, 0.1, 0.9, 1.0 - 0.9, 0.0, 0.0, 1e-8, SEED,
                                0, elements=np.array([0, 1]))
    assert list(q) == [-(0.005 * 0.5), 0.005 * 0.25]
    assert list(m2) == [0.9 * 0.1 + (1.0 - 0.9) * q[0], 0.9 * 0.1 + (1.0 - 0.9) * q[1]]
    assert list(t2) == [0.5 + 0.1 * m2[0], -0.25 + 0.1 * m2[1]]
    t0, m0, _, _, _ = oo.step(theta, m, v, np.zeros(3), oo.MOMENTUM, 2.5, 0.0, 0.1, 0.9, 1.0 - 0.9, 0.0, 0.0, 1e-8, SEED, 0,
                              elements=np.array([0, 1]))
    assert list(m0) == [0.9 * 0.1, 0.9 * 0.1]


@pytest.mark.parametrize("lr", [0.01, 0.3])
def test_first_adam_step_is_lr_times_the_sign(lr):
    """t = 1, zero moments: m' = (1 - b1) q, v' = (1 - b2) q^2 and alpha = lr sqrt(1 - b2) / (1 - b1), so the step is
    lr * q / (|q| + eps / sqrt(1 - b2)): lr * sign(q) to eps / (|q| sqrt(1 - b2)) relative, 3.2e-7 / |q| at the
    defaults - inside 1e-6 for the |q| > 0.5 the case keeps."""
    elements = np.arange(4096, dtype=np.int64)
    theta, z = np.zeros(4096), np.zeros(4096)
    d, sigma, n_c = np.array([1.0, -0.5, 0.75]), 0.05, 6
    gscale, alpha, c1, k1, c2, k2 = es.step_scalars("adam", lr, sigma, n_c, 1, 0.9, 0.999)
    t2, m2, v2, q, st = oo.step(theta, z, z, d, oo.ADAM, gscale, 0.0, alpha, c1, k1, c2, k2, 1e-8, SEED, 0, elements)
    big = np.abs(q) > 0.5
    assert big.sum() > 2000
    np.testing.assert_allclose(st[big], lr * np.sign(q[big]), rtol=1e-6, atol=0)
    assert np.array_equal(t2, st)


# ---------------------------------------------------------------- the Python layer on a recording fake batch
class _FakeBuffer:
    def __init__(self, nbytes):
        self.nbytes, self.ptr, self.host = nbytes, 0xD000 + nbytes, None

    def upload(self, a):
        self.host = np.array(a)
        return self

    def download(self, dtype, shape, offset=0):
        return self.host.astype(dtype).reshape(shape)


class _FakeBatch:
    """Records every library call ES makes; holds the centre and the moments as host arrays."""
    N, M = 2, 2

    def __init__(self, n_weights, n_biases):
        self.calls = []
        G = n_weights + n_biases
        self.nw, self.theta, self.m, self.v = n_weights, np.arange(G, dtype=np.float64), None, None

    def _split(self, a):
        return a[:self.nw].copy(), a[self.nw:].copy()

    def es_create(self, layers):
        self.calls.append(("es_create", list(layers)))

    def es_opt_create(self):
        self.calls.append(("es_opt_create",))
        self.m, self.v = np.zeros_like(self.theta), np.zeros_like(self.theta)

    def es_init(self, seed, generation):
        self.calls.append(("es_init", seed, generation))

    def es_get(self, nw, nb):
        return self._split(self.theta)

    def es_set(self, w, b):
        self.calls.append(("es_set",))
        self.theta = np.concatenate([w, b])

    def es_opt_get(self, nw, nb):
        return self._split(self.m), self._split(self.v)

    def es_opt_set(self, mw, mb, vw, vb):
        self.calls.append(("es_opt_set",))
        self.m, self.v = np.concatenate([mw, mb]), np.concatenate([vw, vb])

    def es_update(self, d, scale, seed, generation):
        self.calls.append(("es_update", np.array(d), scale, seed, generation))

    def es_step(self, d, rule, gscale, decay, alpha, c1, k1, c2, k2, eps, seed, generation, stats_ptr=None):
        self.calls.append(("es_step", np.array(d), rule, gscale, decay, alpha, c1, k1, c2, k2, eps, seed, generation,
                           stats_ptr))

    def sync(self):
        self.calls.append(("sync",))


SMALL = [104, 9, 4]


@pytest.fixture
def fake(monkeypatch):
    monkeypatch.setattr(engine, "DeviceBuffer", _FakeBuffer)
    return _FakeBatch(*es.genome_sizes(SMALL))


@pytest.mark.parametrize("optimizer,rule", [("momentum", 1), ("adam", 2)])
def test_update_passes_exactly_the_documented_scalars(fake, optimizer, rule):
    beta1, beta2, eps, wd = 0.8, 0.99, 1e-6, 0.005
    centre = es.ES(fake, SMALL, 7, optimizer=optimizer, beta1=beta1, beta2=beta2, adam_eps=eps, weight_decay=wd)
    assert [c[0] for c in fake.calls] == ["es_create", "es_opt_create", "es_init"]
    d, lr, sigma, n_c = np.array([0.5, 0.0, -1.0]), 0.07, 0.05, 6
    for t in (1, 2, 3):
        centre.update(d, lr, sigma, n_c, generation=10 + t)
        assert centre.opt_steps == t
        name, got_d, got_rule, gscale, decay, alpha, c1, k1, c2, k2, got_eps, seed, generation, stats_ptr = fake.calls[-1]
        assert name == "es_step" and np.array_equal(got_d, d) and got_rule == rule and (seed, generation) == (7, 10 + t)
        assert gscale == 1.0 / (n_c * sigma) and decay == wd and got_eps == eps
        assert (c1, k1, c2, k2) == (beta1, 1.0 - beta1, beta2, 1.0 - beta2)
        want = lr if optimizer == "momentum" else lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)
        assert alpha == want and stats_ptr == centre._stats.ptr
        assert (gscale, alpha, c1, k1, c2, k2) == oo.scalars(optimizer, lr, sigma, n_c, t, beta1, beta2)
    assert not any(c[0] == "es_update" for c in fake.calls)
    # update keeps its checks, before the step is counted
    for bad in (dict(d=np.array([np.nan])), dict(sigma=0.0), dict(n_c=1), dict(lr=float("inf"))):
        kw = dict(dict(d=d, lr=lr, sigma=sigma, n_c=n_c), **bad)
        with pytest.raises(ValueError):
            centre.update(kw["d"], kw["lr"], kw["sigma"], kw["n_c"], 0)
    assert centre.opt_steps == 3 and fake.calls[-1][0] == "es_step" and fake.calls[-1][12] == 13
    centre._stats.host = np.array([4.0, 0.25, 9.0])
    assert centre.step_stats() == (4.0, 0.25, 9.0) and fake.calls[-1] == ("sync",)


def test_without_an_optimizer_the_calls_are_todays(fake):
    centre = es.ES(fake, SMALL, 7)
    assert [c[0] for c in fake.calls] == ["es_create", "es_init"]
    d = np.array([0.5, -1.0])
    centre.update(d, 0.1, 0.05, 4, 2)
    name, got_d, scale, seed, generation = fake.calls[-1]
    assert name == "es_update" and np.array_equal(got_d, d) and scale == 0.1 / (4 * 0.05) and (seed, generation) == (7, 2)
    assert centre.optimizer is None and centre.opt_steps == 0
    for call in (centre.step_stats, centre.moments, lambda: centre.set_moments(None, None)):
        with pytest.raises(ValueError, match="optimizer"):
            call()
    assert len(fake.calls) == 3


def test_constructor_refuses_before_the_library_is_touched(fake):
    nan, inf = float("nan"), float("inf")
    bad = [("optimizer", dict(optimizer="sgd")), ("optimizer", dict(optimizer="Adam")),
           ("beta1", dict(optimizer="adam", beta1=1.0)), ("beta1", dict(optimizer="momentum", beta1=-0.1)),
           ("beta1", dict(optimizer="adam", beta1=nan)), ("beta2", dict(optimizer="adam", beta2=1.0)),
           ("beta2", dict(optimizer="adam", beta2=-1e-9)), ("beta2", dict(optimizer="adam", beta2=inf)),
           ("adam_eps", dict(optimizer="adam", adam_eps=0.0)), ("adam_eps", dict(optimizer="adam", adam_eps=-1e-8)),
           ("adam_eps", dict(optimizer="adam", adam_eps=nan)), ("adam_eps", dict(optimizer="adam", adam_eps=inf)),
           ("weight_decay", dict(optimizer="adam", weight_decay=-0.005)),
           ("weight_decay", dict(optimizer="adam", weight_decay=nan)),
           ("weight_decay", dict(optimizer="momentum", weight_decay=inf)),
           ("weight_decay", dict(weight_decay=0.005))]
    for word, kw in bad:
        with pytest.raises(ValueError, match=word):
            es.ES(fake, SMALL, 7, **kw)
    assert fake.calls == []
    es.ES(fake, SMALL, 7, optimizer="momentum", beta1=0.0, weight_decay=0.0)        # plain SGD is a momentum of 0


def test_check_es_opt_meta_names_each_field():
    want = es.es_opt_meta("adam", 0.9, 0.999, 1e-8, 0.005, 4)
    assert sorted(want) == ["beta1", "beta2", "eps", "rule", "steps", "weight_decay"]
    G = 17
    meta = {"layers": [1], "seed": 2, "optimizer": dict(want, steps=9)}
    assert es.check_es_opt_meta(meta, want) == 9                         # steps may differ: it is what load restores
    assert es.check_es_opt_meta(meta, want, (2, G), np.float64, G) == 9
    for field, other in (("rule", "momentum"), ("beta1", 0.8), ("beta2", 0.99), ("eps", 1e-6), ("weight_decay", 0.0)):
        with pytest.raises(ValueError, match=field):
            es.check_es_opt_meta(dict(meta, optimizer=dict(want, **{field: other})), want)
        with pytest.raises(ValueError, match=field):
            es.check_es_opt_meta(dict(meta, optimizer={k: v for k, v in want.items() if k != field}), want)
    for steps in (-1, 2.5, None):
        with pytest.raises(ValueError, match="steps"):
            es.check_es_opt_meta(dict(meta, optimizer=dict(want, steps=steps)), want)
    with pytest.raises(ValueError, match="steps"):
        es.check_es_opt_meta(dict(meta, optimizer={k: v for k, v in want.items() if k != "steps"}), want)
    with pytest.raises(ValueError, match="no optimizer block"):
        es.check_es_opt_meta({"layers": [1], "seed": 2}, want)
    with pytest.raises(ValueError, match="has an optimizer block"):
        es.check_es_opt_meta(meta, None)
    assert es.check_es_opt_meta({"layers": [1], "seed": 2}, None) == 0
    with pytest.raises(ValueError, match="shape"):
        es.check_es_opt_meta(meta, want, (2, G + 1), np.float64, G)
    with pytest.raises(ValueError, match="dtype"):
        es.check_es_opt_meta(meta, want, (2, G), np.float32, G)


def test_checkpoint_carries_the_moments_and_refuses_untouched(fake, tmp_path):
    nw, nb = es.genome_sizes(SMALL)
    G = nw + nb
    kw = dict(optimizer="adam", weight_decay=0.005)
    a = es.ES(fake, SMALL, 7, **kw)
    rs = np.random.RandomState(1)
    fake.theta, fake.m, fake.v = rs.uniform(-1, 1, G), rs.uniform(-1, 1, G), rs.uniform(0, 1, G)
    a.opt_steps = 5
    path = a.save(str(tmp_path / "centre.npy"))
    mom = np.load(path + ".opt.npy")
    assert mom.dtype == np.float64 and mom.shape == (2, G)
    assert np.array_equal(_bits(mom[0]), _bits(fake.m)) and np.array_equal(_bits(mom[1]), _bits(fake.v))
    meta = json.load(open(path + ".json"))
    assert meta == {"layers": SMALL, "seed": 7, "optimizer": {"rule": "adam", "beta1": 0.9, "beta2": 0.999, "eps": 1e-8,
                                                               "weight_decay": 0.005, "steps": 5}}
    # moments() / set_moments in the shapes of centre()
    (mW, mB), (vW, vB) = a.moments()
    assert [x.shape for x in mW] == [(9, 104), (4, 9)] and [x.shape for x in vB] == [x.shape for x in a.centre()[1]]
    a.set_moments((vW, vB), (mW, mB))
    assert np.array_equal(fake.m, mom[1]) and np.array_equal(fake.v, mom[0])

    def fresh(**kw2):
        other = _FakeBatch(nw, nb)
        return other, es.ES(other, SMALL, 7, **kw2)

    b2, same = fresh(**kw)
    same.load(path)
    assert same.opt_steps == 5 and np.array_equal(_bits(b2.theta), _bits(fake.theta))
    assert np.array_equal(_bits(b2.m), _bits(mom[0])) and np.array_equal(_bits(b2.v), _bits(mom[1]))
    for word, kw2 in (("has an optimizer block", {}), ("rule", dict(optimizer="momentum", weight_decay=0.005)),
                      ("weight_decay", dict(optimizer="adam")), ("beta2", dict(kw, beta2=0.99)),
                      ("eps", dict(kw, adam_eps=1e-6)), ("beta1", dict(kw, beta1=0.5))):
        b3, other = fresh(**kw2)
        n = len(b3.calls)
        with pytest.raises(ValueError, match=word):
            other.load(path)
        assert len(b3.calls) == n and other.opt_steps == 0, word
    # a checkpoint without an optimizer keeps the sidecar it always had, and an optimizer-carrying ES refuses it
    b4, plain = fresh()
    plain_path = plain.save(str(tmp_path / "plain.npy"))
    assert json.load(open(plain_path + ".json")) == {"layers": SMALL, "seed": 7}
    assert not (tmp_path / "plain.npy.opt.npy").exists()
    b5, wants = fresh(**kw)
    n = len(b5.calls)
    with pytest.raises(ValueError, match="no optimizer block"):
        wants.load(plain_path)
    assert len(b5.calls) == n


# ---------------------------------------------------------------- the loop on the stand-in of tests/test_es.py
class _Batch(eo.EvolutionOracleBatch):
    def state_dict(self):
        return {"episode": self.episode, "lockstep_count": self.lockstep_count}

    def load_state_dict(self, d):
        self.episode, self.lockstep_count = d["episode"], d["lockstep_count"]


N, M, P, TICKS, SIGMA, LR = 4, 3, 4, 6, 0.05, 0.1


def _stand_in(optimizer, log_steps):
    b = _Batch(N, M, 48, 40)
    centre = oo.OptOracleES(b, LAYERS, SEED, optimizer=optimizer, weight_decay=0.005) if optimizer else \
        so.OracleES(b, LAYERS, SEED)
    kw = dict(log_steps=True) if log_steps else {}
    roll = es.ESRollout(b, centre, ["random"] * M, SEED, P, SIGMA, LR, ships=(0, 2), eval_arenas=1, episode_ticks=TICKS, **kw)
    return b, centre, roll


def test_rollout_logs_one_entry_per_stepped_generation_and_round_trips():
    b, centre, roll = _stand_in("adam", True)
    roll.run(2 * TICKS + 2)                                  # inside the third generation's episode
    stepped = [g for g, (_, n_c) in enumerate(roll.weight_log) if n_c >= 2]
    assert roll.generation == 2 and stepped and len(roll.step_log) == len(stepped) == centre.opt_steps
    kinds = [c[0] for c in centre.calls]
    i = kinds.index("fitness")
    assert kinds[i:i + 5] == ["fitness", "update", "step_stats", "assign", "act"]
    assert kinds.count("step_stats") == len(stepped)
    for entry in roll.step_log:
        assert len(entry) == 3 and all(isinstance(x, float) and x > 0 for x in entry)
    assert roll.step_log[-1] == centre.last
    # the update got the scalars of step t
    updates = [c for c in centre.calls if c[0] == "update"]
    for t, c in enumerate(updates, 1):
        d, n_c = roll.weight_log[c[1]]
        assert np.array_equal(c[2], d) and c[3] == oo.scalars("adam", LR, SIGMA, n_c, t, 0.9, 0.999)
    state = roll.state_dict()
    assert state["step_log"] == roll.step_log
    b2, centre2, roll2 = _stand_in("adam", True)
    centre2.theta, centre2.m, centre2.v, centre2.opt_steps = centre.theta.copy(), centre.m.copy(), centre.v.copy(), centre.opt_steps
    roll2.load_state_dict(state)
    assert roll2.step_log == roll.step_log and roll2.state_dict()["step_log"] == state["step_log"]
    assert roll2.generation == 2 and np.array_equal(centre2.member_of, centre.member_of)
    # (the stand-in's batch keeps no arena state: going on bit for bit is tests/test_gpu_es_optimizer.py's resume)
    # the required fields did not change: a state without step_log still loads
    b3, centre3, roll3 = _stand_in("adam", True)
    roll3.load_state_dict({k: v for k, v in state.items() if k != "step_log"})
    assert roll3.step_log == [] and roll3.generation == 2


def test_rollout_defaults_make_todays_calls():
    b, centre, roll = _stand_in(None, False)
    roll.run(2 * TICKS + 1)
    kinds = [c[0] for c in centre.calls]
    i = kinds.index("fitness")
    assert kinds[i:i + 4] == ["fitness", "update", "assign", "act"] and "step_stats" not in kinds
    assert roll.log_steps is False and roll.step_log == [] and "step_log" not in roll.state_dict()
    assert sorted(roll.state_dict()) == sorted(["generation", "episodes", "tick", "fitness_log", "centre_log", "weight_log",
                                                "score_log", "fitness_sum", "fitness_count", "engine"])
    # an optimiser-carrying ES without log_steps: stepped, nothing downloaded
    b2, centre2, roll2 = _stand_in("momentum", False)
    roll2.run(2 * TICKS + 1)
    assert "step_stats" not in [c[0] for c in centre2.calls] and centre2.opt_steps >= 1 and roll2.step_log == []
    # up to the first update both flew the same members of the same fresh centre: the same weights
    assert np.array_equal(roll.weight_log[0][0], roll2.weight_log[0][0])


def test_loop_seed_has_an_untied_pair_in_generation_0():
    """The oracle loop at the sizes of the GPU loop test (N = 8, M = 3, P = 4, T = 10, two evaluation arenas), Adam with
    weight_decay 0.005: the first step of oo.LOOP_SEED has an estimate to step on."""
    b = _Batch(8, 3, 48, 40)
    centre = oo.OptOracleES(b, LAYERS, oo.LOOP_SEED, optimizer="adam", weight_decay=0.005)
    roll = es.ESRollout(b, centre, ["random"] * 3, oo.LOOP_SEED, 4, 0.05, 0.2, ships=(0,), eval_arenas=2, episode_ticks=10,
                        log_steps=True)
    roll.run(11)
    d, n_c = roll.weight_log[0]
    assert roll.generation == 1 and n_c == 4 and d.all(), "both pairs of generation 0 are untied"
    assert len(roll.step_log) == 1 and centre.opt_steps == 1 and centre.m.any() and centre.v.any()
