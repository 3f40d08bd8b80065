"""The member queue of the evolution strategy, the CPU side: the properties of the requeue law on the oracle, the
preconditions that keep the GPU scenarios of tests/test_gpu_es_queue.py from being vacuous, the entry points in header /
binding / library, and ESRollout(auto_reset=True)'s host logic on a call-recording stand-in."""
import ctypes as C

import numpy as np
import pytest

from ofighters_amd import _native as nat
from ofighters_amd import es
from tests import es_queue_oracle as qo
from tests import es_queue_standin as qs
from tests.abi_header import header_symbols
from tests.rollout_standin import fake_device_buffers


def test_entry_points_declared_bound_and_exported():
    declared, L = header_symbols(), C.CDLL(nat.LIB_PATH)
    for s in ("ofx_restart_arenas", "ofx_es_requeue"):
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    assert nat.SIGNATURES["ofx_restart_arenas"][1] == [C.c_void_p, C.c_uint64, C.c_void_p]
    assert nat.SIGNATURES["ofx_es_requeue"][1][3:5] == [C.c_int64, C.c_int64]
    assert nat.SIGNATURES["ofx_es_requeue"][1][-1] == C.c_int32


# ---------------------------------------------------------------- the law on the oracle
def test_a_generation_flies_every_member_exactly_E_times():
    G = qo.GENERATION
    r = qo.generation(**G)
    P, E, total = G["P"], G["E"], G["P"] * G["E"]
    assert (r["count"][:P] == E).all() and r["count"][P] == 0
    assert tuple(r["queue"]) == (total, total)
    # tickets go out in ascending order over the run, and inside a call in ascending (a, i)
    tickets = [t for handed, _, _, _ in r["calls"] for _, _, t in handed]
    assert tickets == list(range(total))
    for handed, refused, _, restarted in r["calls"]:
        where = [(a, i) for a, i, _ in handed]
        assert where == sorted(where)
        assert all(restarted[a] for a, _ in where + refused)
    # completed == total exactly when the last evaluation is banked: at the last call and at no call before it
    completed = [c for _, _, c, _ in r["calls"]]
    assert completed[-1] == total and all(c < total for c in completed[:-1]) and completed == sorted(completed)
    # restarts by death and restarts by clock both occur
    assert r["by_death"] > 0 and r["by_clock"] > 0, (r["by_death"], r["by_clock"])
    # the tail: an arena that restarted once the tickets were out holds idle ships
    assert any(refused for _, refused, _, _ in r["calls"])
    assert (r["member_of"][:, list(G["selected"])] == -1).all()


def test_the_law_cases_are_not_vacuous():
    """On the oracle alone: over the cases tests/test_gpu_es_queue.py uploads, at least one call hands tickets to several
    arenas at once, one runs out in the middle of an arena, one restarted arena holds an idle ship, one banks an
    out-of-range member's neighbours only, and total = 0 refuses everybody."""
    several = mid_arena = idle = skipped = empty = 0
    P = qo.LAW_P
    for n, m in qo.LAW_SHAPES:
        arena_mask, member_of, queue_mask = qo.law_inputs(n, m)
        last = np.arange(n * m, dtype=np.int32).reshape(n, m) % 7 - 2
        for nxt, completed, total in qo.law_queues(arena_mask, queue_mask):
            mo = member_of.copy()
            queue = np.array([nxt, completed], np.int64)
            s, c = np.zeros(P + 1, np.int64), np.zeros(P + 1, np.int32)
            handed, refused = qo.requeue(arena_mask, mo, queue_mask, last, P, total, queue, s, c, 1)
            several += len({a for a, _, _ in handed}) > 1
            mid_arena += bool({a for a, _, _ in handed} & {a for a, _ in refused})
            idle += bool(((member_of == -1) & (arena_mask[:, None] != 0)).any())
            out_of_range = (member_of[arena_mask != 0] < -1) | (member_of[arena_mask != 0] > P)
            skipped += bool(out_of_range.any()) and int(c.sum()) == int((~out_of_range & (member_of[arena_mask != 0] >= 0)).sum())
            empty += total == 0 and not handed and len(refused) == int(queue_mask[arena_mask != 0].sum())
            assert queue[0] == nxt + len(handed) and (mo[arena_mask == 0] == member_of[arena_mask == 0]).all()
            assert queue[1] == completed + int(c[:P].sum())
    assert several and mid_arena and idle and skipped and empty, (several, mid_arena, idle, skipped, empty)


# ---------------------------------------------------------------- ESRollout(auto_reset=True) on the stand-in
N, M, P, E, TICKS, POLL, SIGMA, LR, SEED = 4, 3, 6, 2, 9, 4, 0.05, 0.1, 31


def _rollout(monkeypatch, done_at=(), **kw):
    log = []
    made = fake_device_buffers(monkeypatch)
    eng, centre = qs.QueueEngine(log, N, M), qs.QueueES(log, done_at)
    args = dict(ships=(0, 2), eval_arenas=1, episode_ticks=TICKS, episodes_per_generation=E)
    args.update(kw)
    roll = es.ESRollout(eng, centre, ["random"] * M, SEED, P, SIGMA, LR, **args)
    return log, made, eng, centre, roll


def _kinds(log):
    return [c[0] for c in log]


def test_auto_reset_calls_in_order(monkeypatch):
    log, made, eng, centre, roll = _rollout(monkeypatch, done_at=(1,), auto_reset=True, poll_every=POLL)
    # construction: spawn, the held assignment, then a generation begins
    assert _kinds(log) == ["spawn", "assign", "queue_begin", "restart_arenas", "requeue"]
    held, queue_mask = log[1][1], log[2][1]
    want_q = np.zeros((N, M), np.uint8)
    want_q[:N - 1, [0, 2]] = 1                                   # `ships` in the first N - eval_arenas arenas
    assert np.array_equal(queue_mask, want_q) and log[2][2:] == (P, E * P)
    want_held = np.full((N, M), -1, np.int32)
    want_held[N - 1, [0, 2]] = P                                 # the evaluation arena holds the centre throughout
    assert np.array_equal(held, want_held) and log[1][2] == P
    assert log[3] == ("restart_arenas", None) and log[4] == ("requeue", False)
    restart_mask = made[0].held                                  # `ships` in EVERY arena
    assert np.array_equal(restart_mask, np.repeat([[1, 0, 1]], N, axis=0))
    del log[:]
    roll.run(2 * POLL + 1)
    # every lock-step starts with restart_finished on the restart mask and the clock, then requeue(bank=True)
    step = [("restart_finished", made[0].ptr, TICKS), ("requeue", True)]
    fly = lambda t, g: [("bots", t), ("act", SIGMA, g), ("step",)]
    want = []
    for t in range(2 * POLL + 1):
        want += step
        if t and t % POLL == 0:
            want.append(("poll",))
        if t == 2 * POLL:                                        # the second poll reports completed == total
            want += [("fitness_host",), ("update", 0, P), ("queue_begin",), ("restart_arenas", None), ("requeue", False)]
        want += fly(t, 1 if t == 2 * POLL else 0)
    got = [c[:1] if c[0] == "queue_begin" else c for c in log]
    assert got == want
    assert roll.generation == 1 and roll.generation_log == [(2 * POLL, P, 1)]
    assert len(roll.fitness_log) == len(roll.centre_log) == len(roll.weight_log) == 1
    assert roll.score_log == [] and eng.episode == 0 and "restart_random" not in _kinds(log)
    assert roll.total == E * P


def test_polls_only_at_multiples_of_poll_every(monkeypatch):
    log, _, _, _, roll = _rollout(monkeypatch, auto_reset=True, poll_every=3)
    del log[:]
    roll.run(10)
    ticks, t = [], -1
    for c in log:
        if c[0] == "bots":
            t = c[1]
        if c[0] == "poll":
            ticks.append(t + 1)                                  # a poll stands before its lock-step's bots
    assert ticks == [3, 6, 9] and roll.generation == 0


def test_bad_arguments_are_refused_before_any_engine_call(monkeypatch):
    for kw, name in ((dict(auto_reset=1), "auto_reset"), (dict(auto_reset="yes"), "auto_reset"),
                     (dict(auto_reset=True, poll_every=0), "poll_every"), (dict(poll_every=2.0), "poll_every"),
                     (dict(auto_reset=True, poll_every=True), "poll_every")):
        log = []
        with pytest.raises(ValueError, match=name):
            es.ESRollout(qs.QueueEngine(log, N, M), qs.QueueES(log), ["random"] * M, SEED, P, SIGMA, LR, **kw)
        assert log == [], kw
    log = []
    with pytest.raises(ValueError, match="dist"):
        es.ESRollout(qs.QueueEngine(log, N, M), qs.QueueES(log), ["random"] * M, SEED, P, SIGMA, LR, auto_reset=True,
                     dist=object())
    assert log == []


def test_option_off_makes_the_calls_of_a_rollout_without_the_argument(monkeypatch):
    def run(**kw):
        log, _, _, _, roll = _rollout(monkeypatch, **kw)
        roll.run(2 * TICKS * E + 2)
        return [tuple(x.tolist() if isinstance(x, np.ndarray) else x for x in c) for c in log], roll
    plain, r0 = run()
    off, r1 = run(auto_reset=False, poll_every=5)
    assert plain == off and "restart_random" in _kinds(plain) and "requeue" not in _kinds(plain)
    assert r0.generation == r1.generation == 2 and r0.generation_log == r1.generation_log == []
    # P may exceed N * len(ships) with the option on
    log, _, _, _, big = _rollout(monkeypatch, auto_reset=True, ships=(1,))
    assert big.P == P > N * 1


def test_state_dict_refuses_a_differing_option_by_field(monkeypatch):
    log, _, eng, centre, roll = _rollout(monkeypatch, done_at=(0,), auto_reset=True, poll_every=POLL)
    roll.run(POLL + 2)                                           # inside the second generation, between two polls
    d = roll.state_dict()
    assert d["auto_reset"] is True and d["poll_every"] == POLL and d["generation"] == 1
    assert d["queue"] == (E * P, E * P - 1) and d["generation_log"] == [(POLL, P, 1)] and d["generation_tick"] == POLL
    assert np.array_equal(d["member_of"], centre.member_of)
    for kw, field in ((dict(auto_reset=True, poll_every=POLL + 1), "poll_every"), (dict(auto_reset=False), "auto_reset"),
                      (dict(auto_reset=False, poll_every=POLL), "auto_reset")):
        log2, _, _, _, other = _rollout(monkeypatch, **kw)
        del log2[:]
        with pytest.raises(ValueError, match=field):
            other.load_state_dict(d)
        assert log2 == [] and other.generation == 0 and other.tick == 0, "nothing is touched"
    # a state written with the option off is refused by a rollout with it on
    _, _, _, _, off = _rollout(monkeypatch)
    log3, _, _, _, on = _rollout(monkeypatch, auto_reset=True, poll_every=POLL)
    assert "auto_reset" not in off.state_dict() and "poll_every" not in off.state_dict()
    with pytest.raises(ValueError, match="auto_reset"):
        on.load_state_dict(off.state_dict())
    with pytest.raises(ValueError, match="'queue'"):
        on.load_state_dict({k: v for k, v in d.items() if k != "queue"})
    # and the same options load: the saved tickets and counters replace the fresh generation's
    log4, _, eng4, _, same = _rollout(monkeypatch, auto_reset=True, poll_every=POLL)
    del log4[:]
    same.load_state_dict(d)
    assert _kinds(log4) == ["load_autoreset", "load_queue", "load_fitness"]
    assert log4[1][2] == d["queue"] and np.array_equal(log4[1][1], d["member_of"])
    assert same.generation == 1 and same.tick == POLL + 2 and same.generation_log == d["generation_log"]
    d2 = same.state_dict()
    assert sorted(d2) == sorted(d) and d2["generation_tick"] == POLL
