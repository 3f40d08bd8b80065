"""Seeded evolution strategies, the CPU side: the noise law, pair_weights, the refusals of the Python layer, the entry
points in header / binding / library, and ESRollout's host logic on an oracle-backed stand-in (the centre held by the
oracle).  The kernels are held to the same oracle in tests/test_gpu_es.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import pyoracle
from ofighters_amd import _native as nat
from ofighters_amd import es
from tests import es_oracle as so
from tests import evolution_oracle as eo
from tests.abi_header import header_symbols

LAYERS = [8 + 2 * 48 * 40, 9, 4]
SEED = 0x0E512345


def test_entry_points_declared_bound_and_exported():
    declared, L = header_symbols(), C.CDLL(nat.LIB_PATH)
    for s in ("ofx_es_create", "ofx_es_destroy", "ofx_es_init", "ofx_es_get", "ofx_es_set", "ofx_es_member", "ofx_es_act",
              "ofx_es_fitness", "ofx_es_update"):
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    assert nat.SIGNATURES["ofx_es_act"][1][2:6] == [C.c_int64, C.c_double, C.c_uint64, C.c_uint32]
    assert nat.SIGNATURES["ofx_es_update"][1][2:] == [C.c_int64, C.c_double, C.c_uint64, C.c_uint32]
    import ofighters_amd
    assert ofighters_amd.ES is es.ES and ofighters_amd.ESRollout is es.ESRollout
    assert ofighters_amd.pair_weights is es.pair_weights


def test_stream_id_is_12_distinct_and_stated_once():
    """The ES stream stands in ofx_rng.h beside the enum of the twelve older streams (which tests/test_rng_streams.py
    holds to 0 .. 11): its id is 12, the oracle's, no other stream's, and no other file of the library defines it."""
    import glob
    import os
    import re
    from tests.abi_header import ROOT
    csrc = os.path.join(ROOT, "ofighters_amd", "csrc")
    text = open(os.path.join(csrc, "ofx_rng.h")).read()
    define = r"^\s*OFX_ES_STREAM\s*=\s*(\d+)\s*,"
    assert re.findall(define, text, re.M) == [str(so.STREAM_ES)] == ["12"]
    others = [int(v) for v in re.findall(r"^\s*OFX_STREAM_\w+\s*=\s*(\d+)\s*,", text, re.M)]
    assert len(others) == 12 and so.STREAM_ES not in others
    anywhere = re.compile(r"#\s*define\s+OFX_ES_STREAM|\bOFX_ES_STREAM\s*=[^=]")
    files = [f for f in glob.glob(os.path.join(csrc, "*")) if f.endswith((".h", ".hip", ".cpp", ".c", ".hpp"))]
    files.append(os.path.join(ROOT, "include", "ofx.h"))
    assert len(files) > 10
    for f in files:
        if os.path.basename(f) != "ofx_rng.h":
            assert not anywhere.search(open(f).read()), os.path.basename(f)


# ---------------------------------------------------------------- the noise law
def test_noise_hand_computed_values():
    top = 2.0 - 2.0 ** -31                                   # (2^33 - 2) / 2^32
    assert so.eps_of_words([0, 0, 0, 0]) == -top
    assert so.eps_of_words([0xFFFFFFFF] * 4) == top
    # S = 1 + 2^31 + (2^32 - 1) + 5 = 6442450949;  S - (2^33 - 2) = -2147483641
    assert so.eps_of_words([1, 1 << 31, 0xFFFFFFFF, 5]) == -2147483641 / 4294967296
    assert so.eps_of_words([0xFFFFFFFF, 0xFFFFFFFF, 0, 0]) == 0.0        # the middle of the range
    assert so.eps_of_words([0xFFFFFFFF, 0xFFFFFFFF, 1, 0]) == 2.0 ** -32  # one step of the grid


def test_noise_is_exactly_symmetric_and_bounded():
    rs = np.random.RandomState(1)
    r = rs.randint(0, 1 << 32, (20000, 4), dtype=np.uint64).astype(np.uint32)
    e = so.eps_of_words(r)
    assert np.array_equal(so.eps_of_words(~r), -e)           # complemented words negate eps, bit for bit
    assert (np.abs(e) < 2.0).all()
    # variance (1 - 2^-64) / 3: the sample variance of n draws of this law (fourth moment 0.3) has a standard error of
    # sqrt((0.3 - 1/9) / n) = 0.0031 at n = 20000; five of them
    assert abs(e.var() - 1.0 / 3.0) < 0.016 and abs(e.mean()) < 5 * np.sqrt(1 / 3 / 20000)


def test_noise_scalar_path_agrees_with_the_array_path():
    elements = np.array([0, 1, 77, 34680, 2880120], np.int64)
    for pair, generation in ((0, 0), (3, 2), (16383, 1000)):
        got = so.eps(SEED, pair, elements, generation)
        for e, v in zip(elements, got):
            assert v == so.eps_scalar(SEED, pair, e, generation)
            r = pyoracle.philox(pair, int(e), generation, so.STREAM_ES, SEED)
            assert v == so.eps_of_words(np.asarray(r, np.uint32))
    # another pair, another generation, another stream than a fresh genome's: other draws
    assert so.eps(SEED, 0, elements, 0)[0] != so.eps(SEED, 1, elements, 0)[0]
    assert so.eps(SEED, 0, elements, 0)[0] != so.eps(SEED, 0, elements, 1)[0]


def test_oracle_members_mirror_each_other():
    theta = eo.fresh(LAYERS, SEED, 0, 0)
    P, sigma, gen = 6, 0.05, 3
    e = np.arange(theta.size, dtype=np.int64)
    for i in range(P // 2):
        noise = so.eps(SEED, i, e, gen)
        plus, minus = np.multiply(sigma, noise), np.multiply(-sigma, noise)
        assert np.array_equal(plus, -minus)                  # the two terms are exact negatives of each other
        assert np.array_equal(so.member(theta, SEED, 2 * i, P, sigma, gen), theta + plus)
        assert np.array_equal(so.member(theta, SEED, 2 * i + 1, P, sigma, gen), theta + minus)
    assert np.array_equal(so.member(theta, SEED, P, P, sigma, gen), theta)
    # a sample of elements gives the full vector's values
    pick = np.array([0, 5, 3848 * 9 - 1, 3848 * 9, theta.size - 1])
    assert np.array_equal(so.member(theta[pick], SEED, 3, P, sigma, gen, elements=pick), so.member(theta, SEED, 3, P, sigma, gen)[pick])
    # update: zero weights leave the centre's value, one pair moves it along that pair's noise
    assert np.array_equal(so.update(theta, [0.0, 0.0], 0.5, SEED, gen), theta + 0.0)
    assert np.array_equal(so.update(theta, [0.0, 2.0], 0.5, SEED, gen), theta + 0.5 * (2.0 * so.eps(SEED, 1, e, gen)))


# ---------------------------------------------------------------- pair_weights
def test_pair_weights_hand_worked():
    # means 3, 1 | 2, 2 | 0, 5; slot 6 is the centre and is ignored.  Ascending average ranks: member 4 -> 0, 1 -> 1,
    # 2 and 3 -> 2.5, 0 -> 4, 5 -> 5;  u = rank / 5 - 0.5
    s, c = np.array([6, 1, 4, 2, 0, 5, 99], np.int64), np.array([2, 1, 2, 1, 1, 1, 7], np.int32)
    d, n_c = es.pair_weights(s, c)
    assert n_c == 6 and d.dtype == np.float64 and d.shape == (3,)
    assert list(d) == [(4 / 5 - 0.5) - (1 / 5 - 0.5), 0.0, (0 / 5 - 0.5) - (5 / 5 - 0.5)]
    assert d[2] == -1.0
    # without the centre's slot: the same
    d2, n2 = es.pair_weights(s[:6], c[:6])
    assert np.array_equal(d, d2) and n2 == 6


def test_pair_weights_ties_and_incomplete_pairs():
    s, c = np.array([6, 1, 4, 2, 0, 5, 99], np.int64), np.array([2, 0, 2, 1, 1, 1, 7], np.int32)
    d, n_c = es.pair_weights(s, c)                           # member 1 was never flown: pair 0 is incomplete
    # ranks among members 2, 3, 4, 5: 4 -> 0, 2 and 3 -> 1.5, 5 -> 3
    assert n_c == 4 and list(d) == [0.0, 0.0, -1.0]
    # all means equal, a single complete pair that ties, nobody flown: all zeros
    for s, c, n in (([4, 2, 2, 6], [2, 1, 1, 3], 4), ([3, 3, 1, 0], [1, 1, 1, 0], 2), ([0, 0, 0, 0], [0, 0, 0, 0], 0),
                    ([5, 1, 0, 0], [1, 0, 0, 1], 0)):
        d, n_c = es.pair_weights(np.array(s, np.int64), np.array(c, np.int32))
        assert n_c == n and not d.any()
    # a single complete pair: +-1
    d, n_c = es.pair_weights(np.array([2, -3], np.int64), np.array([1, 1], np.int32))
    assert n_c == 2 and list(d) == [1.0]


def test_pair_weights_properties_and_the_oracle():
    rs = np.random.RandomState(4)
    for _ in range(60):
        n_pairs = int(rs.randint(1, 9))
        s = rs.randint(-6, 7, 2 * n_pairs + 1).astype(np.int64)
        c = rs.randint(0, 3, 2 * n_pairs + 1).astype(np.int32)
        d, n_c = es.pair_weights(s, c)
        want, want_n = so.pair_weights(s, c)
        assert n_c == want_n and np.array_equal(d, want)
        assert (np.abs(d) <= 1.0).all()
        complete = (c[:-1].reshape(-1, 2) > 0).all(axis=1)
        assert n_c == 2 * complete.sum() and not d[~complete].any()
        mean = s[:-1].reshape(-1, 2)[complete] / c[:-1].reshape(-1, 2)[complete]
        assert not d[complete][mean[:, 0] == mean[:, 1]].any()          # a tied pair weighs exactly 0
        assert (np.sign(d[complete]) == np.sign(mean[:, 0] - mean[:, 1])).all()
        # swapping every pair's two members negates the weights, exactly
        swap = np.arange(2 * n_pairs).reshape(-1, 2)[:, ::-1].ravel()
        d2, n2 = es.pair_weights(s[:-1][swap], c[:-1][swap])
        assert n2 == n_c and np.array_equal(d2, -d)
    with pytest.raises(ValueError):
        es.pair_weights(np.zeros(1, np.int64), np.zeros(1, np.int32))
    with pytest.raises(ValueError):
        es.pair_weights(np.zeros(4, np.int64), np.zeros(5, np.int32))


# ---------------------------------------------------------------- the loop on the stand-in
class _Batch(eo.EvolutionOracleBatch):
    def state_dict(self):
        return {"episode": self.episode, "lockstep_count": self.lockstep_count}

    def load_state_dict(self, d):
        self.episode, self.lockstep_count = d["episode"], d["lockstep_count"]


N, M, P, TICKS, SIGMA, LR = 4, 3, 4, 6, 0.05, 0.1


def _stand_in(ships=(0, 2), base=0, eval_arenas=1):
    b = _Batch(N, M, 48, 40, arena_base=base)
    centre = so.OracleES(b, LAYERS, SEED)
    roll = es.ESRollout(b, centre, ["random"] * M, SEED, P, SIGMA, LR, ships=ships, eval_arenas=eval_arenas,
                        episode_ticks=TICKS)
    return b, centre, roll


@pytest.fixture(scope="module")
def stand_in_run():
    b, centre, roll = _stand_in()
    roll.run(3 * TICKS + 1)                                  # the third generation ends at the head of lock-step 18
    return b, centre, roll


def test_es_rollout_on_the_stand_in(stand_in_run):
    b, centre, roll = stand_in_run
    assert roll.observe is False and roll.generation == 3 and len(roll.score_log) == 3
    assert len(roll.fitness_log) == len(roll.centre_log) == len(roll.weight_log) == 3
    calls = centre.calls
    kinds = [c[0] for c in calls]
    # act on every lock-step, once, before the step, with the rollout's sigma and the running generation
    acts = [c for c in calls if c[0] == "act"]
    assert [c[1] for c in acts] == list(range(3 * TICKS + 1))
    assert all(c[2] == SIGMA for c in acts)
    assert [c[3] for c in acts] == [0] * TICKS + [1] * TICKS + [2] * TICKS + [3]
    # fitness at every episode end (reset: one episode per generation)
    assert [c for c in calls if c[0] == "fitness"] == [("fitness", True)] * 3
    # the order at an episode end: ... act(5) | fitness, update, assign | act(6) ...
    i = kinds.index("fitness")
    assert calls[i - 1][:2] == ("act", TICKS - 1)
    flew_complete = [n_c >= 2 for _, n_c in roll.weight_log]
    assert flew_complete[0], "the stand-in's first generation has a complete pair"
    assert kinds[i:i + 4] == ["fitness", "update", "assign", "act"]
    # an update per generation that had something to learn from, on the generation that just flew, with
    # scale = lr / (n_c * sigma) and the d of pair_weights
    updates = [c for c in calls if c[0] == "update"]
    assert [c[1] for c in updates] == [g for g in range(3) if flew_complete[g]]
    for c in updates:
        d, n_c = roll.weight_log[c[1]]
        assert np.array_equal(c[2], d) and c[3] == LR / (n_c * SIGMA)
    # member_of by the formula, the last arena flies the centre, re-assigned after every generation
    assigns = [c for c in calls if c[0] == "assign"]
    assert len(assigns) == 4
    for gen, (_, got, p) in enumerate(assigns):
        want = np.full((N, M), -1, np.int32)
        for a in range(N):
            for k, ship in enumerate((0, 2)):
                want[a, ship] = P if a == N - 1 else ((0 + a) * 2 + k + gen) % P
        assert p == P and np.array_equal(got, want) and np.array_equal(got, roll.assignment(gen))
    for best, mean in roll.fitness_log:
        assert best >= mean
    # the centre's log is the evaluation arena's two ships' mean banked score
    assert all(isinstance(v, float) for v in roll.centre_log)
    s, c = centre.fitness_host()
    assert c[P] == 2 and roll.centre_log[-1] == s[P] / c[P]


def test_es_rollout_is_reproducible_and_keyed_by_global_arena(stand_in_run):
    _, centre, roll = stand_in_run
    _, centre2, roll2 = _stand_in()
    roll2.run(3 * TICKS + 1)
    assert roll.fitness_log == roll2.fitness_log and roll.centre_log == roll2.centre_log
    assert np.array_equal(centre.theta, centre2.theta)
    assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] for x, y in zip(roll.weight_log, roll2.weight_log))
    _, _, roll3 = _stand_in(base=5, eval_arenas=0)
    assert roll3.assignment(1)[1, 2] == ((5 + 1) * 2 + 1 + 1) % P
    assert (roll3.assignment(0) != P).all() and roll3.centre_log == []


def test_es_rollout_evolved_ships_fly_the_decoded_output():
    """A lock-step of the stand-in: the evolved ships' actions are the decode of the oracle forward on the oracle's
    member, the others the bots'."""
    b, centre, roll = _stand_in(ships=(1,), eval_arenas=1)
    bots = [a.bot_actions(np.full(M, nat.BOT_RANDOM, np.int32), SEED, g, 0) for g, a in enumerate(b.arenas)]
    want = []
    for g, a in enumerate(b.arenas):
        sm, lm = a.rasterise()
        head, _ = a.obs_head()
        m = int(roll.assignment(0)[g, 1])
        assert m == (P if g == N - 1 else g % P)
        w = so.member(centre.theta, SEED, m, P, SIGMA, 0)
        want.append(eo.decode(eo.forward(LAYERS, w, head[1], sm, lm), 48, 40))
    b.bot_actions(roll.behaviours, SEED, tick=0)
    roll.policy(b)
    for g in range(N):
        assert np.array_equal(b._acts[g][1], want[g]) and want[g][0] == 1
        assert np.array_equal(b._acts[g][[0, 2]], bots[g][[0, 2]])


def test_es_rollout_state_dict_round_trips():
    b, centre, roll = _stand_in()
    roll.run(TICKS + 2)                                      # inside the second generation's episode
    d = roll.state_dict()
    assert d["generation"] == 1 and d["tick"] == TICKS + 2 and len(d["weight_log"]) == 1 and len(d["centre_log"]) == 1
    b2, centre2, roll2 = _stand_in()
    centre2.theta = centre.theta.copy()                      # ES.load's part
    roll2.load_state_dict(d)
    d2 = roll2.state_dict()
    assert sorted(d) == sorted(d2)
    for k in d:
        if k == "weight_log":
            assert len(d[k]) == len(d2[k]) and all(np.array_equal(u[0], v[0]) and u[1] == v[1] for u, v in zip(d[k], d2[k]))
        elif k == "score_log":
            assert len(d[k]) == len(d2[k]) and all(np.array_equal(u, v) for u, v in zip(d[k], d2[k]))
        elif isinstance(d[k], np.ndarray):
            assert np.array_equal(d[k], d2[k]), k
        else:
            assert d[k] == d2[k], k
    assert np.array_equal(centre2.member_of, centre.member_of) and np.array_equal(centre2.member_of, roll.assignment(1))
    with pytest.raises(ValueError, match="'tick'"):
        roll2.load_state_dict({k: v for k, v in d.items() if k != "tick"})


def test_python_layer_refuses():
    b = _Batch(2, 2, 48, 40)
    centre = so.OracleES(b, LAYERS, SEED)
    ok = dict(P=4, sigma=0.05, lr=0.1)
    with pytest.raises(ValueError, match="dist"):
        es.ESRollout(b, centre, ["random"] * 2, SEED, dist=object(), **ok)
    for P in (3, 0, 1, -2, 2.5):                             # odd, too small, not an integer
        with pytest.raises(ValueError, match="P must"):
            es.ESRollout(b, centre, ["random"] * 2, SEED, **dict(ok, P=P))
    for sigma in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            es.ESRollout(b, centre, ["random"] * 2, SEED, **dict(ok, sigma=sigma))
    with pytest.raises(ValueError, match="lr"):
        es.ESRollout(b, centre, ["random"] * 2, SEED, **dict(ok, lr=float("nan")))
    with pytest.raises(ValueError, match="ships"):
        es.ESRollout(b, centre, ["random"] * 2, SEED, ships=(2,), **ok)
    with pytest.raises(ValueError, match="eval_arenas"):
        es.ESRollout(b, centre, ["random"] * 2, SEED, eval_arenas=2, **ok)
    with pytest.raises(ValueError):
        es.ESRollout(b, centre, ["random"] * 2, SEED, episodes_per_generation=0, **ok)
    with pytest.raises(ValueError):
        es.ESRollout(b, centre, ["random"] * 2, SEED, observe=True, **ok)
    # the assignment: P is a value, P + 1 and -2 are not
    a = np.full((3, 2), -1, np.int64)
    a[1, 1] = 4
    assert es.check_member_assignment(a, 3, 2, 4).dtype == np.int32
    for v in (5, -2):
        bad = a.copy()
        bad[2, 0] = v
        with pytest.raises(ValueError, match="outside"):
            es.check_member_assignment(bad, 3, 2, 4)
    with pytest.raises(ValueError):
        es.check_member_assignment(a, 2, 3, 4)


def test_es_checkpoint_refuses_by_field():
    layers, seed = [104, 9, 4], 11
    meta = es.es_meta(layers, seed)
    shape = (sum(es.genome_sizes(layers)),)
    es.check_es_meta(meta, shape, np.float64, layers, seed)
    for field, other in (("layers", [104, 8, 4]), ("seed", 12)):
        with pytest.raises(ValueError, match=field):
            es.check_es_meta(dict(meta, **{field: other}), shape, np.float64, layers, seed)
        with pytest.raises(ValueError, match=field):
            es.check_es_meta({k: v for k, v in meta.items() if k != field}, shape, np.float64, layers, seed)
    with pytest.raises(ValueError, match="shape"):
        es.check_es_meta(meta, (shape[0] + 1,), np.float64, layers, seed)
    with pytest.raises(ValueError, match="dtype"):
        es.check_es_meta(meta, shape, np.float32, layers, seed)
