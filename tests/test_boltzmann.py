"""Boltzmann exploration, the CPU side: the float64 reference of tests/boltzmann_oracle.py samples what it says it
samples, the temperature follows the ladder's rule, and TrainingRollout(boltzmann=...) makes the calls it documents -
and, with the option off, exactly the calls it made before the option existed (tests/golden/play_calls.json, recorded
from that commit by tests/record_play_calls.py)."""
import json
import math
import os

import numpy as np
import pytest

from oracle import pyoracle
from tests import boltzmann_oracle as bo
from tests import play_standin as ps
from tests.rollout_standin import fake_device_buffers

SEED = 0x0B01752A
# chi-square quantiles at an upper tail of p = 1e-4 (scipy.stats.chi2.isf(1e-4, df)); the seeds are fixed, so the tests
# are deterministic
CHI2_1E4 = {31: 69.10569228986719, 1: 15.136705226623397}
TICKS = 20000


def _chi2(counts, p):
    e = p * counts.sum()
    return float(((counts - e) ** 2 / e).sum())


# ---- the vectorised Philox is pyoracle.philox --------------------------------------------------------------------
def test_array_philox_is_the_oracles_word_for_word():
    rng = np.random.RandomState(5)
    cs = rng.randint(0, 2 ** 32, size=(300, 4), dtype=np.uint64)
    cs[:8] = [[0, 0, 0, 0], [2 ** 32 - 1] * 4, [1, 0, 0, 6], [0, 1, 0, 6], [0, 0, 1, 7], [7, 79999, 5, 6], [3, 40000, 2 ** 31, 6],
              [2 ** 31, 2 ** 31 + 1, 9, 7]]
    for seed in (0, SEED, 2 ** 64 - 1, 0x123456789ABCDEF0):
        got = bo.philox_words(seed, cs[:, 0], cs[:, 1], cs[:, 2], cs[:, 3])
        for k, c in enumerate(cs):
            assert np.array_equal(got[k], pyoracle.philox(int(c[0]), int(c[1]), int(c[2]), int(c[3]), seed)), (seed, c)


def test_noise_map_counters_and_words():
    """Pixel (x, y) of ship i takes word x & 3 of block i * (W*H/4) + (y*W + x) / 4; the array path is the scalar one."""
    W, H, G, i, tick = 8, 4, 11, 3, 9
    fast, slow = bo.noise_map(SEED, G, i, tick, W, H), bo.noise_map(SEED, G, i, tick, W, H, scalar=True)
    assert fast.shape == (H, W) and np.array_equal(fast, slow)
    for (x, y) in ((0, 0), (3, 0), (4, 0), (7, 3), (5, 2)):
        r = pyoracle.philox(G, i * (W * H // 4) + (y * W + x) // 4, tick, 6, SEED)[x & 3]
        w = (float(r) + 0.5) / 2.0 ** 32
        assert fast[y, x] == -math.log(-math.log1p(-w))
    many = bo.noise_map(SEED, G, i, np.array([9, 10]), W, H)
    assert many.shape == (2, H, W) and np.array_equal(many[0], fast) and not np.array_equal(many[1], fast)
    full = bo.noise_map(SEED, 2, 1, 4)                       # a ship's whole map: blocks 40000 .. 79999
    assert full.shape == (400, 400)
    r = pyoracle.philox(2, 40000 + (399 * 400 + 397) // 4, 4, 6, SEED)[397 & 3]
    assert full[399, 397] == bo.gumbel(np.array([r]))[0]
    a = bo.action_noise(SEED, G, i, tick)
    assert np.array_equal(a, bo.gumbel(pyoracle.philox(G, i, tick, 7, SEED)[:2]))
    assert np.array_equal(bo.action_noise(SEED, G, i, np.array([tick, tick + 1]))[0], a)


def test_gumbel_tails_are_finite_and_ordered():
    g = bo.gumbel(bo.edge_words())
    assert np.all(np.isfinite(g)) and np.all(np.diff(g) < 0)          # g falls as the word grows
    assert abs(g[0] - 33 * math.log(2)) < 1e-9 and abs(g[-1] + math.log(33 * math.log(2))) < 1e-9


# ---- the sampler samples softmax(Q / T) --------------------------------------------------------------------------
def test_pointer_distribution_is_the_softmax():
    W, H, T = 8, 4, np.float32(0.7)
    logits = (np.random.RandomState(3).rand(H, W) * 3.0).astype(np.float32)
    g = bo.noise_map(SEED, 5, 1, np.arange(TICKS), W, H)              # [TICKS][H][W]
    ref = (np.float64(T) * g + logits.astype(np.float64)).astype(np.float32)
    pick = ref.reshape(TICKS, -1).argmax(axis=1)
    for t in (0, 1, TICKS - 1):                                        # the batched form is choose_pointer's
        px, py = bo.choose_pointer(logits, T, g[t])
        assert py * W + px == pick[t]
    counts = np.bincount(pick, minlength=W * H).astype(np.float64)
    assert _chi2(counts, bo.softmax(logits, T)) < CHI2_1E4[31]
    assert _chi2(counts, np.full(W * H, 1.0 / (W * H))) > 10 * CHI2_1E4[31]   # and the test can tell: not uniform


def test_action_distribution_is_the_softmax():
    act, T = np.array([0.3, -0.2], np.float32), np.float32(0.5)
    g = bo.action_noise(SEED, 2, 0, np.arange(TICKS))
    p = bo.perturbed(act[None, :], T, g)
    ones = int((p[:, 1] > p[:, 0]).sum())
    assert [bo.choose_action(act, T, g[t]) for t in range(5)] == [int(v) for v in (p[:5, 1] > p[:5, 0])]
    counts = np.array([TICKS - ones, ones], np.float64)
    assert _chi2(counts, bo.softmax(act, T)) < CHI2_1E4[1]
    assert _chi2(counts, np.array([0.5, 0.5])) > 10 * CHI2_1E4[1]


def test_zero_temperature_is_the_first_maximum():
    heat = np.zeros((4, 8), np.float32)
    heat[1, 5] = heat[1, 6] = heat[3, 0] = 2.0                         # three equal maxima: the first in C order wins
    g = bo.noise_map(SEED, 0, 0, 0, 8, 4)
    assert bo.choose_pointer(heat, 0.0, g) == (5, 1)
    assert bo.choose_pointer(heat, 0.0, None) == (5, 1)               # no noise is read at all
    assert np.array_equal(bo.perturbed(heat, 0.0, g), heat)
    assert bo.choose_action([1.0, 1.0], 0.0, None) == 0 and bo.choose_action([1.0, 2.0], 0.0, None) == 1
    assert bo.choose_action([2.0, 1.0], 0.0, None) == 0
    ref = bo.perturbed(heat, 0.0, None)
    assert bo.accepted(ref, 1 * 8 + 5, 0.0) and bo.accepted(ref, 3 * 8 + 0, 0.0) and not bo.accepted(ref, 0, 0.0)


def test_temperature_follows_the_ladder():
    eps, tau = 0.37, 1.75
    T = bo.temperatures(tau, eps, [1.0, 2.5, np.inf, 0.0])
    assert T.dtype == np.float32
    assert T[0] == np.float32(tau) * np.float32(eps)                   # exponent 1: epsilon itself, no pow
    assert T[1] == np.float32(tau) * np.float32(math.pow(eps, 2.5))
    assert T[2] == 0.0                                                 # +inf: a greedy arena
    assert T[3] == np.float32(tau)                                     # exponent 0: eps_a = 1
    assert np.array_equal(bo.temperatures(tau, eps, n=3), np.full(3, np.float32(tau) * np.float32(eps), np.float32))
    assert np.array_equal(bo.temperatures(0.0, eps, [1.0, 2.5]), np.zeros(2, np.float32))


def test_acceptance_rule():
    ref = np.array([[1.0, 3.0, 2.0], [3.0 - 1e-6, 0.0, 3.0]], np.float32)
    T = 0.5
    tol = 2 * T * bo.GUMBEL_ABS_ERR + 4 * float(np.spacing(np.float32(3.0)))
    assert bo.tolerance(ref, T) == tol and bo.GUMBEL_ABS_ERR <= 1e-4
    assert bo.accepted(ref, 1, T) and bo.accepted(ref, 5, T) and bo.accepted(ref, 3, T)
    assert not bo.accepted(ref, 2, T) and not bo.accepted(ref, 0, T)


# ---- TrainingRollout(boltzmann=...) ------------------------------------------------------------------------------
BAD = [1.0, (1.0,), (1.0, 2.0, 3.0), (-1.0, 1.0), (1.0, -0.5), (float("nan"), 1.0), (1.0, float("inf")), ("1", 1.0),
       (True, 1.0), (None, 1.0), "ab", (1.0, 1e39)]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_bad_arguments_are_refused_before_any_engine_call(monkeypatch, bad):
    from ofighters_amd.rollout import TrainingRollout
    made = fake_device_buffers(monkeypatch)
    e = ps.PlayEngine()
    with pytest.raises(ValueError, match="boltzmann"):
        TrainingRollout(e, ps.PlayTrainer(), ["idle", "idle"], seed=3, boltzmann=bad)
    assert e.calls == 0 and e.log == [] and made == []


def test_good_arguments_become_a_pair_of_floats(monkeypatch):
    from ofighters_amd.rollout import TrainingRollout
    fake_device_buffers(monkeypatch)
    for arg, want in (((0, 0), (0.0, 0.0)), ([0.5, 2], (0.5, 2.0)), (np.array([1.5, 0.25], np.float32), (1.5, 0.25))):
        r = TrainingRollout(ps.PlayEngine(), ps.PlayTrainer(), ["idle", "idle"], seed=3, boltzmann=arg)
        assert r.boltzmann == want and all(type(v) is float for v in r.boltzmann)
    assert TrainingRollout(ps.PlayEngine(), ps.PlayTrainer(), ["idle", "idle"], seed=3).boltzmann is None


def _run(monkeypatch, trainer_kw, rollout_kw):
    import ofighters_amd.rollout as ro
    return json.loads(json.dumps(ps.run_case(ro, lambda: fake_device_buffers(monkeypatch), trainer_kw, rollout_kw)))


@pytest.mark.parametrize("name", sorted(ps.OFF_CASES))
def test_option_off_makes_the_recorded_calls(monkeypatch, name):
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "play_calls.json")) as f:
        want = json.load(f)
    assert sorted(want) == sorted(ps.OFF_CASES)
    tkw, rkw = ps.OFF_CASES[name]
    assert _run(monkeypatch, tkw, rkw) == want[name]
    assert _run(monkeypatch, tkw, dict(rkw, boltzmann=None)) == want[name]


@pytest.mark.parametrize("name", sorted(ps.OFF_CASES))
def test_option_on_replaces_the_choice_by_one_call(monkeypatch, name):
    """The log with the option on is the log without it, with `forward` + `explore` (or `act`) replaced by one
    `act_boltzmann` that takes the same epsilon, seed, tick, collecting flag and FULL policy mask; captures, masks,
    replays and everything else stay."""
    tkw, rkw = ps.OFF_CASES[name]
    off, on = _run(monkeypatch, tkw, rkw), _run(monkeypatch, tkw, dict(rkw, boltzmann=(0.5, 3.0)))
    want, log, k = [], off["log"], 0
    while k < len(log):
        c = log[k]
        if isinstance(c, list) and c[0] == "forward":
            x = log[k + 1]
            assert x[0] == "explore" and x[5] == c[2]
            want.append(["act_boltzmann", c[1], x[1], 0.5, 3.0, x[2], x[3], x[4], x[5]])
            k += 2
        elif isinstance(c, list) and c[0] == "act":
            want.append(["act_boltzmann", c[1], c[2], 0.5, 3.0] + c[3:])
            k += 1
        else:
            want.append(c)
            k += 1
    assert on["log"] == want
    assert on["replays"] == off["replays"] and on["capture_tick"] == off["capture_tick"] == ps.STEPS
    acts = [c for c in on["log"] if isinstance(c, list) and c[0] == "act_boltzmann"]
    assert len(acts) == ps.STEPS and [c[6] for c in acts] == list(range(ps.STEPS))      # tick = capture_tick
    assert [c[7] for c in acts] == [s + 1 < 5 for s in range(ps.STEPS)]                # collecting_steps = 5
    assert not any(isinstance(c, list) and c[0] in ("forward", "explore", "act") for c in on["log"])
    valued = bool(tkw.get("actor_priorities"))
    assert any(isinstance(c, list) and c[0] == "capture_valued" for c in on["log"]) == valued
    assert any(isinstance(c, list) and c[0] == "capture" for c in on["log"]) == (not valued)
    if "eval_arenas" in rkw:            # the call takes the full policy mask, the capture the learning mask
        k = on["log"].index(acts[0])
        assert on["log"][k + 1][0] == "capture_valued" and on["log"][k + 1][2] != acts[0][8]
        assert on["log"][k + 2] == ["actions", acts[0][8]]


# ---- the checkpoint fingerprint ----------------------------------------------------------------------------------
def _ck_engine():
    from tests.checkpoint_standin import CheckpointEngine

    class BoltzmannCheckpointEngine(CheckpointEngine):
        def policy_act_boltzmann(self, w, eps, tau_act, tau_ptr, seed, tick=None, collecting=False, ship_mask_ptr=None):
            self.log.append("act_boltzmann:%d:%d" % (tick, collecting))
    return BoltzmannCheckpointEngine


def test_fingerprint_carries_the_key_only_when_on(monkeypatch, tmp_path):
    from ofighters_amd import checkpoint
    from tests.checkpoint_standin import ROLLOUT_KEYS, standins
    r_off = standins(monkeypatch, tmp_path, engine=_ck_engine())[0]
    r_on = standins(monkeypatch, tmp_path, engine=_ck_engine(), boltzmann=(0.5, 3))[0]
    off, on = checkpoint.rollout_fingerprint(r_off), checkpoint.rollout_fingerprint(r_on)
    assert sorted(off) == sorted(ROLLOUT_KEYS) and "boltzmann" not in off
    assert on["boltzmann"] == [0.5, 3.0] and {k: v for k, v in on.items() if k != "boltzmann"} == off


@pytest.mark.parametrize("saved,restored", [(None, (0.5, 3.0)), ((0.5, 3.0), None), ((0.5, 3.0), (0.5, 2.0))])
def test_checkpoint_of_one_mode_is_refused_under_the_other(monkeypatch, tmp_path, saved, restored):
    from tests.checkpoint_standin import standins
    a = standins(monkeypatch, tmp_path, engine=_ck_engine(), boltzmann=saved)[0]
    a.run(6)
    path = str(tmp_path / "ck")
    a.checkpoint(path)
    b, _, _, uploads = standins(monkeypatch, tmp_path, engine=_ck_engine(), boltzmann=restored)
    with pytest.raises(ValueError, match="boltzmann"):
        b.restore(path)
    assert uploads == []                                                # nothing was touched
    c = standins(monkeypatch, tmp_path, engine=_ck_engine(), boltzmann=saved)[0]
    c.restore(path)                                                     # the same mode restores
    assert c.total_steps == a.total_steps and c.capture_tick == a.capture_tick
