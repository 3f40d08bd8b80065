"""The exploration ladder and evaluation arenas without a device: the host arithmetic of ofighters_amd/exploration.py, the
inputs of the device test (how far they keep from a last-bit flip of pow), the binding's entries, and TrainingRollout's
fingerprint / checkpoint under the options on the stand-ins of tests/checkpoint_standin.py."""
import math

import numpy as np
import pytest

from ofighters_amd import _native as nat
from ofighters_amd.exploration import apex_exponents, score_groups
from tests import ladder_oracle as lo
from tests import checkpoint_standin as base

LADDER_KEYS = ("epsilon_ladder", "eval_arenas", "total_arenas", "score_bands")


# ------------------------------------------------------------------------------------------------ apex_exponents
def test_apex_exponents_values():
    e = apex_exponents(10, 7.0, 0, 10)
    assert e.dtype == np.float64 and e.shape == (10,)
    assert e.tolist() == [1.0 + 7.0 * g / 9.0 for g in range(10)] and e[0] == 1.0 and e[-1] == 8.0
    e = apex_exponents(10, 7.0, 0, 10, eval_arenas=3)              # L = 7 rungs, then three greedy arenas
    assert e[:7].tolist() == [1.0 + 7.0 * g / 6.0 for g in range(7)] and e[6] == 8.0
    assert np.isposinf(e[7:]).all()
    assert apex_exponents(5, 0.0, 0, 5).tolist() == [1.0] * 5       # alpha 0: everyone at epsilon itself
    assert apex_exponents(5, 0, 0, 5, 2).tolist() == [1.0, 1.0, 1.0, math.inf, math.inf]
    assert apex_exponents(np.int64(6), np.float32(2.0), np.int32(0), 6, np.int64(1))[4] == 3.0   # numpy scalars are numbers


def test_apex_exponents_is_keyed_by_the_global_arena():
    whole = apex_exponents(8, 7.0, 0, 8, eval_arenas=2)
    for cut in (1, 4, 6, 7):                                        # also a shard that is all greedy, and one that has none
        halves = np.concatenate([apex_exponents(8, 7.0, 0, cut, 2), apex_exponents(8, 7.0, cut, 8 - cut, 2)])
        assert halves.tobytes() == whole.tobytes()
    thirds = np.concatenate([apex_exponents(12, 3.0, b, 4) for b in (0, 4, 8)])
    assert thirds.tobytes() == apex_exponents(12, 3.0, 0, 12).tobytes()


def test_apex_exponents_one_learning_arena():
    assert apex_exponents(1, 7.0, 0, 1).tolist() == [1.0]
    assert apex_exponents(4, 7.0, 0, 4, eval_arenas=3).tolist() == [1.0, math.inf, math.inf, math.inf]
    assert apex_exponents(4, 7.0, 2, 2, eval_arenas=3).tolist() == [math.inf, math.inf]


@pytest.mark.parametrize("kw", [
    dict(alpha=-0.5), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(alpha=True), dict(alpha="7"),
    dict(eval_arenas=-1), dict(eval_arenas=8), dict(eval_arenas=9), dict(eval_arenas=True), dict(eval_arenas=2.0),
    dict(total_arenas=True), dict(total_arenas=8.0), dict(total_arenas=0), dict(n=False), dict(n=0), dict(n=4.0),
    dict(arena_base=-1), dict(arena_base=1.0), dict(arena_base=5)])           # arenas [5, 9) of 8
def test_apex_exponents_refuses(kw):
    a = dict(total_arenas=8, alpha=7.0, arena_base=0, n=4, eval_arenas=2)
    a.update(kw)
    with pytest.raises(ValueError) as err:
        apex_exponents(a["total_arenas"], a["alpha"], a["arena_base"], a["n"], a["eval_arenas"])
    key = next(iter(kw))
    assert (key if key != "arena_base" or kw[key] != 5 else "outside") in str(err.value)


# ---------------------------------------------------------------------------------------------------- score_groups
def test_score_groups_values_and_sharding():
    g = score_groups(18, 0, 18, 4, 2)                               # 16 learning arenas in 4 bands of 4, then the eval group
    assert g.dtype == np.int32 and g.tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 2
    assert score_groups(16, 0, 16, 4, 0).tolist() == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
    assert score_groups(6, 0, 6, 1, 0).tolist() == [0] * 6
    uneven = score_groups(10, 0, 10, 3, 0)                          # bands need not divide: contiguous, sizes within one
    assert (np.diff(uneven) >= 0).all() and sorted(np.bincount(uneven).tolist()) == [3, 3, 4]
    whole = score_groups(18, 0, 18, 4, 2)
    for cut in (5, 9, 16, 17):
        assert np.concatenate([score_groups(18, 0, cut, 4, 2), score_groups(18, cut, 18 - cut, 4, 2)]).tolist() == whole.tolist()
    assert score_groups(4, 0, 4, 1, 3).tolist() == [0, 1, 1, 1]     # one learning arena
    for bad in (dict(bands=0), dict(bands=17), dict(bands=True), dict(bands=2.0), dict(eval_arenas=18)):
        a = dict(bands=4, eval_arenas=2)
        a.update(bad)
        with pytest.raises(ValueError):
            score_groups(18, 0, 18, a["bands"], a["eval_arenas"])


# ------------------------------------------------------------------------------- the inputs of the device test
def test_device_test_inputs_keep_away_from_a_flip_and_use_every_rung():
    """The device's pow may differ from glibc's in the last bit; u is a multiple of 2^-32, so the comparison can only
    flip where eps_a * 2^32 is within an ulp (< 1e-6 here) of an integer.  No ship is left out of this check."""
    from oracle import pyoracle
    ex = lo.ladder()
    assert ex[0] == 1.0 and ex[lo.N - lo.EVAL - 1] == 8.0 and np.isposinf(ex[lo.N - lo.EVAL:]).all()
    assert lo.flip_distance(lo.EPSILONS, ex) >= 1e-4
    hits = {}
    for eps, tick in zip(lo.EPSILONS, (7, 8)):
        hit, _ = lo.explore(pyoracle, lo.M, eps, ex, lo.SEED, lo.ARENA_BASE, tick)
        assert not hit[lo.N - lo.EVAL:].any()
        hits[eps] = lo.band_hits(hit)
    sizes = [lo.M * min(lo.BAND, lo.N - lo.EVAL - a) for a in range(0, lo.N - lo.EVAL, lo.BAND)]
    assert all(0 < h < s for h, s in zip(hits[0.9], sizes)), hits         # every band both explores and does not
    assert 0 < hits[0.4][0] < sizes[0] and hits[0.4][-1] == 0, hits       # from a fifth of the first band down to nobody
    assert all(lo_ <= hi for lo_, hi in zip(hits[0.4], hits[0.9]))
    # the special cases of the law
    assert lo.arena_eps(0.3, 1.0) == 0.3 and lo.arena_eps(0.0, 0.0) == 1.0 and lo.arena_eps(0.3, math.inf) is None
    assert lo.arena_eps(0.0, 2.5) == 0.0 and lo.arena_eps(1.0, 8.0) == 1.0


def test_binding_carries_the_new_entries():
    sig = nat.SIGNATURES
    assert sig["ofx_policy_epsilon_ladder"] == (nat._i, [nat._vp, nat._vp])
    assert sig["ofx_policy_epsilon_ladder_host"] == (nat._i, [nat._vp, nat._vp])
    import ctypes as C
    assert sig["ofx_episode_scores_grouped"] == (nat._i, [nat._vp, nat._vp, C.c_int32, nat._vp])
    for name in ("ofx_policy_epsilon_ladder", "ofx_policy_epsilon_ladder_host", "ofx_episode_scores_grouped"):
        assert hasattr(nat.lib(), name)
    assert sig["ofx_policy_explore"][1][1] is C.c_double and len(sig["ofx_policy_explore"][1]) == 8   # unchanged


# ------------------------------------------------------------------ TrainingRollout on the stand-ins: fingerprint, checkpoint
class _LadderEngine(base.CheckpointEngine):
    """The stand-in engine with the two calls the options add."""
    ladder = None

    def policy_epsilon_ladder(self, expo):
        self.log.append("ladder")
        self.ladder = None if expo is None else np.array(expo, np.float64)

    def episode_scores_grouped(self, group_buf, n_groups):
        grp = np.asarray(group_buf.data)
        out = np.zeros((n_groups, self.M + 1), np.int64)
        for a in range(self.N):
            if 0 <= grp[a] < n_groups:
                out[grp[a], :self.M] += 10 * a + np.arange(self.M) + self.episode
                out[grp[a], self.M] += 1
        return out


def _standins(monkeypatch, tmp_path, **kw):
    kw.setdefault("engine_kw", {"N": 6})
    return base.standins(monkeypatch, tmp_path, engine=_LadderEngine, **kw)


ON = dict(epsilon_ladder=7.0, eval_arenas=2, score_bands=2)


def test_fingerprint_gains_keys_only_when_an_option_is_on(tmp_path, monkeypatch):
    from ofighters_amd.checkpoint import rollout_fingerprint
    r, e, _, _ = _standins(monkeypatch, tmp_path)
    assert tuple(sorted(rollout_fingerprint(r))) == tuple(sorted(base.ROLLOUT_KEYS))
    assert e.ladder is None and "ladder" not in e.log and r._learn_mask is r._mask and r.rung_log == [] and r.eval_scores == []
    r.run(45)
    assert r.rung_log == [] and len(r.score_log) == 1
    for kw, want in ((ON, dict(epsilon_ladder=7.0, eval_arenas=2, total_arenas=6, score_bands=2)),
                     (dict(eval_arenas=1), dict(epsilon_ladder=None, eval_arenas=1, total_arenas=6, score_bands=5)),
                     (dict(epsilon_ladder=0.0), dict(epsilon_ladder=0.0, eval_arenas=0, total_arenas=6, score_bands=6)),
                     (dict(epsilon_ladder=2, total_arenas=12, engine_kw={"N": 6, "arena_base": 6}, eval_arenas=3),
                      dict(epsilon_ladder=2.0, eval_arenas=3, total_arenas=12, score_bands=5))):
        r, e, _, _ = _standins(monkeypatch, tmp_path, **kw)
        fp = rollout_fingerprint(r)
        assert tuple(sorted(fp)) == tuple(sorted(base.ROLLOUT_KEYS + LADDER_KEYS))
        assert {k: fp[k] for k in LADDER_KEYS} == want
        # what the constructor derived: the ladder on the engine, the second mask, the groups
        expo = apex_exponents(want["total_arenas"], want["epsilon_ladder"] or 0.0, e.arena_base, e.N, want["eval_arenas"])
        assert e.ladder.tobytes() == expo.tobytes()
        greedy = np.isinf(expo)
        if want["eval_arenas"]:
            assert r._learn_mask is not r._mask
            assert not r._learn_mask.data[greedy].any() and np.array_equal(r._learn_mask.data[~greedy], r._mask.data[~greedy])
            assert np.array_equal(r._mask.data, r.policy_mask) and r.policy_mask[greedy].any()
        else:
            assert r._learn_mask is r._mask
        assert r._groups.data.tolist() == score_groups(want["total_arenas"], e.arena_base, e.N, want["score_bands"],
                                                       want["eval_arenas"]).tolist()
        assert r.n_groups == want["score_bands"] + (1 if want["eval_arenas"] else 0) <= e.N


@pytest.mark.parametrize("kw,word", [(dict(epsilon_ladder=-1.0), "alpha"), (dict(epsilon_ladder=float("nan")), "alpha"),
                                     (dict(eval_arenas=6), "eval_arenas"), (dict(eval_arenas=True), "eval_arenas"),
                                     (dict(eval_arenas=1.5), "eval_arenas"), (dict(eval_arenas=1, score_bands=0), "score_bands"),
                                     (dict(epsilon_ladder=1.0, score_bands=2.5), "score_bands"),
                                     (dict(epsilon_ladder=1.0, total_arenas=4), "outside")])
def test_rollout_refuses_bad_arguments_before_any_engine_call(tmp_path, monkeypatch, kw, word):
    calls = []
    monkeypatch.setattr(_LadderEngine, "spawn_random", lambda self, seed: calls.append("spawn"))
    with pytest.raises(ValueError) as err:
        _standins(monkeypatch, tmp_path, **kw)
    assert word in str(err.value) and calls == []


def test_rung_log_and_checkpoint_round_trip(tmp_path, monkeypatch):
    from ofighters_amd import checkpoint
    r, e, t, _ = _standins(monkeypatch, tmp_path, **ON)
    r.run(93)                                                        # two episode ends
    assert len(r.rung_log) == 2 == len(r.score_log) and r.rung_log[0].shape == (3, e.M + 1) and r.rung_log[0].dtype == np.int64
    assert [g[:, -1].tolist() for g in r.rung_log] == [[2, 2, 2]] * 2          # two bands of two arenas, two greedy arenas
    want = [(10 * 4 + ep) + (10 * 5 + ep) for ep in (1, 2)]                    # ship 0 of arenas 4 and 5, per episode
    assert r.eval_scores == [w / 2.0 for w in want]
    path = str(tmp_path / "ck")
    r.checkpoint(path)
    rd = checkpoint.Reader(path)
    assert rd.array("rollout/rung_log").shape == (2, 3, e.M + 1) and np.array_equal(rd.array("rollout/rung_log"), np.array(r.rung_log))
    assert {k: rd.manifest["rollout_fingerprint"][k] for k in LADDER_KEYS} == dict(epsilon_ladder=7.0, eval_arenas=2,
                                                                                   total_arenas=6, score_bands=2)
    r2, e2, t2, _ = _standins(monkeypatch, tmp_path, **ON)
    r2.restore(path)
    assert np.array_equal(r2.rung_log, r.rung_log) and r2.eval_scores == r.eval_scores
    e2.seen, r2._seen_done.cleared = e.seen.copy(), False
    r.run(40), r2.run(40)
    assert len(r2.rung_log) == 3 and np.array_equal(r2.rung_log, r.rung_log)
    # with the options off the section is not written
    r0, _, _, _ = _standins(monkeypatch, tmp_path)
    r0.run(50)
    r0.checkpoint(str(tmp_path / "off"))
    assert "rollout/rung_log" not in checkpoint.Reader(str(tmp_path / "off")).sections


@pytest.mark.parametrize("other,keys", [(dict(epsilon_ladder=3.0, eval_arenas=2, score_bands=2), ["epsilon_ladder"]),
                                        (dict(epsilon_ladder=7.0, eval_arenas=1, score_bands=2), ["eval_arenas"]),
                                        (dict(epsilon_ladder=7.0, eval_arenas=2, score_bands=3), ["score_bands"]),
                                        (dict(epsilon_ladder=None, eval_arenas=2, score_bands=2), ["epsilon_ladder"]),
                                        (dict(epsilon_ladder=7.0, eval_arenas=2, score_bands=2, total_arenas=12),
                                         ["total_arenas"]),
                                        ({}, list(LADDER_KEYS))])
def test_restore_refuses_other_ladder_arguments_before_any_upload(tmp_path, monkeypatch, other, keys):
    r, _, _, _ = _standins(monkeypatch, tmp_path, **ON)
    r.run(50)
    path = str(tmp_path / "ck")
    r.checkpoint(path)
    r2, e2, t2, up2 = _standins(monkeypatch, tmp_path, **other)
    before = (e2.memory.copy(), t2.w.copy(), r2.tick)
    with pytest.raises(ValueError) as err:
        r2.restore(path)
    for k in keys:
        assert "rollout.%s " % k in str(err.value), str(err.value)
    assert str(err.value).count(" here, ") == len(keys)
    assert up2 == [] and r2.tick == before[2] and np.array_equal(e2.memory, before[0]) and np.array_equal(t2.w, before[1])
    # and the other way round: a checkpoint of a run without the options is refused under them
    if not other:
        r2.run(50)
        r2.checkpoint(path)
        r3, _, _, up3 = _standins(monkeypatch, tmp_path, **ON)
        with pytest.raises(ValueError) as err:
            r3.restore(path)
        assert all("rollout.%s " % k in str(err.value) for k in LADDER_KEYS) and up3 == []
