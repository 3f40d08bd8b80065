"""DeviceTrainer(global_sampling=True) in the training loop: every replay fits one minibatch drawn from all arenas'
memories, runs repeat bit for bit, a checkpoint resumes bit for bit and is refused by a per-arena trainer, and the default
trainer's replay() issues the calls it always issued."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, SEED = 16, 2, 0x0F160061
FIT = 96
CONFIGS = {"uniform": {}, "per_nstep_packed": dict(prioritized=True, n_step=3, packed_memory=True, per_beta_steps=10)}
TOTAL, SPLIT = 40, 22


def _build(cfg, global_sampling=True):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N, M)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=FIT,
                       global_sampling=global_sampling, **CONFIGS[cfg])
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0, 1), episode_ticks=20, collecting_steps=5,
                           replay_every=3)
    return b, tr, roll


def _record(b, names):
    """Wrap the batch's methods `names`: every call appends (name, args, result) to the returned list."""
    log = []
    for name in names:
        def wrap(fn, name=name):
            def call(*a, **kw):
                out = fn(*a, **kw)
                log.append((name, a, out))
                return out
            return call
        setattr(b, name, wrap(getattr(b, name)))
    return log


def _state(b, tr, roll):
    from tests.train_state import training_state as ckpt_state
    s = ckpt_state(b, tr, roll)                          # weights, moments, losses, counters, arenas, rows, masses, frames
    s["blob"] = b.replay_export(0, N).tobytes()          # ... and mmax, which only the blob shows
    return s


_RUNS = {}


def _run(cfg):
    """The run that never stops, once per configuration: its states at SPLIT and TOTAL and what its replays fitted."""
    if cfg not in _RUNS:
        b, tr, roll = _build(cfg)
        log = _record(b, ["replay_sample_global", "replay_gather_list_into", "dqn_fit", "dqn_fit_weighted",
                          "replay_update_priorities_list", "replay_count", "replay_sample", "replay_sample_prioritized"])
        out = {}
        for stop in (SPLIT, TOTAL):
            roll.run(stop - roll.tick)
            seen = len(log)
            out[stop] = _state(b, tr, roll)
            del log[seen:]                               # the inspections' own calls (replay_count) are not the trainer's
        rows_arg = ("replay_gather_list_into", "replay_update_priorities_list")
        out["log"] = [(name, a[2] if name in rows_arg else None, a[5] if name.startswith("dqn_fit") else None,
                       r[3:] if name == "replay_sample_global" else None) for name, a, r in log]
        b.close()
        _RUNS[cfg] = out
    return _RUNS[cfg]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_every_replay_fits_one_global_minibatch(cfg):
    ref = _run(cfg)
    per = bool(CONFIGS[cfg].get("prioritized"))
    log = ref["log"]
    assert not [x for x in log if x[0] in ("replay_count", "replay_sample", "replay_sample_prioritized")]
    per_replay = 4 if per else 3
    fits = 0
    seen = set()
    i = 0
    while i < len(log):
        name, _, _, drawn = log[i]
        assert name == "replay_sample_global"
        n, eligible = drawn
        assert n == min(FIT, eligible)
        seen.add(n == FIT)
        if n == 0:
            i += 1
            continue
        names = [x[0] for x in log[i:i + per_replay]]
        assert names == ["replay_sample_global", "replay_gather_list_into", "dqn_fit_weighted" if per else "dqn_fit"] + \
            (["replay_update_priorities_list"] if per else [])
        assert log[i + 1][1] == n and log[i + 2][2] == n and (not per or log[i + 3][1] == n)
        fits += 1
        i += per_replay
    assert fits >= 8 and fits == ref[TOTAL]["fit_steps"] and seen == {False, True}   # fewer than, and at least, FIT rows
    assert np.isfinite(np.array(ref[TOTAL]["losses"])).all()
    if per:
        from tests import ckpt_blob
        d = ckpt_blob.decode(np.frombuffer(ref[TOTAL]["blob"], np.uint8))
        assert len(set(d["mmax"].tolist())) == 1 and d["mmax"][0] > 1.0               # levelled over the arenas
        assert (d["mass"] != 1.0).sum() >= FIT // 2


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_two_runs_and_a_resumed_run_are_bit_identical(tmp_path, cfg):
    ref = _run(cfg)
    b, tr, roll = _build(cfg)
    roll.run(SPLIT)
    assert tr.fit_steps >= 3 and ref[TOTAL]["fit_steps"] >= tr.fit_steps + 3
    here = _state(b, tr, roll)
    assert [k for k in here if here[k] != ref[SPLIT][k]] == []                       # a second run: == weights and losses
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    b.close()
    del b, tr, roll
    b, tr, roll = _build(cfg)
    m = roll.restore(path)
    assert m["counters"]["tick"] == SPLIT and m["trainer_fingerprint"]["global_sampling"] is True
    after = _state(b, tr, roll)
    assert [k for k in after if after[k] != ref[SPLIT][k]] == []
    roll.run(TOTAL - SPLIT)
    end = _state(b, tr, roll)
    assert [k for k in end if end[k] != ref[TOTAL][k]] == []      # names what differs; every entry is compared with ==
    assert end == ref[TOTAL]
    b.close()
    # the other sampler refuses the checkpoint, naming the key, and stays as it was
    b, tr, roll = _build(cfg, global_sampling=False)
    roll.run(3)
    before = _state(b, tr, roll)
    with pytest.raises(ValueError) as err:
        roll.restore(path)
    assert "trainer.global_sampling " in str(err.value)
    assert _state(b, tr, roll) == before
    b.close()


CALLS = ["sync", "policy_blend_weights", "dqn_targets_double_into"] + \
    [n for n in ("replay_count replay_sample replay_sample_prioritized replay_gather_valid_into replay_gather_nstep_into "
                 "replay_window_weights_into replay_update_priorities replay_sample_global replay_gather_list_into "
                 "replay_update_priorities_list dqn_fit dqn_fit_weighted dqn_fit_robust dqn_fit_reference").split()]
BEFORE = {  # what replay() called on the batch before global sampling existed, in order
    "uniform": ["replay_count", "replay_sample", "sync", "replay_gather_valid_into", "dqn_fit"],
    "per_nstep_packed": ["replay_count", "replay_sample_prioritized", "sync", "replay_gather_nstep_into",
                         "replay_window_weights_into", "dqn_fit_weighted", "replay_update_priorities"],
}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_the_default_replay_issues_the_calls_it_issued_before(cfg):
    b, tr, roll = _build(cfg, global_sampling=False)
    roll.run(8)
    assert "global_sampling" not in tr.fingerprint()
    log = _record(b, CALLS)
    steps = tr.fit_steps
    assert tr.replay() is not None and tr.fit_steps == steps + 1
    assert [x[0] for x in log] == BEFORE[cfg]
    b.close()
    b, tr, roll = _build(cfg, global_sampling=True)
    roll.run(8)
    log = _record(b, CALLS)
    assert tr.replay() is not None
    per = cfg != "uniform"
    assert [x[0] for x in log] == ["replay_sample_global", "replay_gather_list_into", "dqn_fit_weighted" if per else "dqn_fit"] + \
        (["replay_update_priorities_list"] if per else [])
    b.close()
