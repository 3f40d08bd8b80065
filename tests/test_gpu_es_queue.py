"""The member queue of the evolution strategy on the device: ofx_restart_arenas against the CPU model, ofx_es_requeue
against the numpy law (tests/es_queue_oracle.py), their refusals, and ESRollout(auto_reset=True) lock-step by lock-step
against a twin whose requeue is the numpy law on downloaded arrays, through three generations and through a stop and a
resume in fresh handles.  Every comparison is `==` on integers or on bits."""
import numpy as np
import pytest

from tests import autoreset_oracle as ao
from tests import es_queue_oracle as qo
from tests import repeat_oracle as ro
from tests.es_cases import H, NIN, SEED, W, bits as _bits
from tests.test_gpu_auto_reset import _against_model, _differences, _state

pytestmark = pytest.mark.gpu


def _dev(a):
    from ofighters_amd import DeviceBuffer
    a = np.ascontiguousarray(a)
    return DeviceBuffer(a.nbytes).upload(a)


# ---------------------------------------------------------------- 1. ofx_restart_arenas against the oracle
@pytest.mark.parametrize("m", (3, 13))
def test_restart_arenas_against_the_oracle(m):
    from ofighters_amd import ArenaBatch
    n, seed = 5, 777 + m
    b = ArenaBatch(n, m, width=W, height=H, **ro.REWARDS)
    b.spawn_random(seed)
    mo = qo.Model(seed, n, m, np.ones((n, m), bool), 0, width=W, height=H)
    beh = ao.behaviours(m)
    for t in range(30):                                          # the rule without a clock: it only marks the dead
        b.restart_finished(seed, None, 0)
        mo.restart_finished()
        b.bot_actions(beh, seed, tick=t)
        b.step()
        mo.step(t)
    before, auto0 = _state(b), b.autoreset_state()
    assert _against_model(before, mo.snapshot()) == []
    assert np.array_equal(auto0["dead_once"], mo.dead_once) and auto0["dead_once"].any(), "no mark to clear"
    assert before["F_SCORE"].any() and before["n_lasers"].any()

    def check(what):
        st, auto = _state(b), b.autoreset_state()
        assert _against_model(st, mo.snapshot()) == [], what
        for k in ("arena_episode", "dead_once", "restarted"):
            assert np.array_equal(auto[k], getattr(mo, k)), (what, k)
        return st, auto

    mask = np.array([1, 1, 0, 1, 1], np.uint8)                   # the first and the last arena set, one clear
    b.restart_arenas(seed, _dev(mask))
    mo.restart_arenas(mask)
    st, auto = check("mask")
    assert np.array_equal(auto["restarted"], mask)
    for k in st:                                                 # the unselected arena keeps every bit
        assert np.array_equal(st[k][2], before[k][2]), k
    assert np.array_equal(auto["dead_once"][2], auto0["dead_once"][2])
    assert auto["arena_episode"][2] == auto0["arena_episode"][2]
    assert not auto["dead_once"][mask != 0].any() and (st["F_TIME"][mask != 0] == 0).all()
    assert np.array_equal(st["F_LAST_SCORES"][mask != 0], before["F_SCORE"][mask != 0])
    b.restart_arenas(seed)                                       # the NULL mask: every arena
    mo.restart_arenas(None)
    st, auto = check("null mask")
    assert (auto["restarted"] == 1).all() and not auto["dead_once"].any() and (st["F_TIME"] == 0).all()
    assert b.episode == 0
    b.close()


# ---------------------------------------------------------------- 2. the requeue law
@pytest.mark.parametrize("n,m", qo.LAW_SHAPES)
def test_requeue_law(n, m):
    from ofighters_amd import ArenaBatch, _native as nat
    P = qo.LAW_P
    b = ArenaBatch(n, m, width=W, height=H, **ro.REWARDS)
    b.spawn_random(SEED)
    beh = ao.behaviours(m)
    for t in range(12):
        b.bot_actions(beh, SEED, tick=t)
        b.step()
    arena_mask, member_of, queue_mask = qo.law_inputs(n, m)
    b.restart_arenas(SEED, _dev(arena_mask))                     # `restarted` becomes the arbitrary mask
    assert np.array_equal(b.autoreset_state()["restarted"], arena_mask)
    last = b.get(nat.F_LAST_SCORES)
    assert n == 1 or last[arena_mask != 0].any()
    rs = np.random.RandomState(n + m)
    sum0, count0 = rs.randint(-50, 50, P + 1).astype(np.int64), rs.randint(0, 5, P + 1).astype(np.int32)
    d_member, d_mask = _dev(member_of), _dev(queue_mask)
    d_queue, d_sum, d_count = _dev(np.zeros(2, np.int64)), _dev(sum0), _dev(count0)
    for nxt, completed, total in qo.law_queues(arena_mask, queue_mask):
        for bank in (0, 1):
            want = dict(member=member_of.copy(), queue=np.array([nxt, completed], np.int64), sum=sum0.copy(),
                        count=count0.copy())
            qo.requeue(arena_mask, want["member"], queue_mask, last, P, total, want["queue"], want["sum"], want["count"],
                       bank)
            for rep in range(3):                                 # the same uploaded state, the same bytes
                b.sync()
                d_member.upload(member_of), d_queue.upload(np.array([nxt, completed], np.int64))
                d_sum.upload(sum0), d_count.upload(count0)
                b.es_requeue(d_member.ptr, d_mask.ptr, P, total, d_queue, d_sum, d_count, bank)
                b.sync()
                got = dict(member=d_member.download(np.int32, (n, m)), queue=d_queue.download(np.int64, (2,)),
                           sum=d_sum.download(np.int64, (P + 1,)), count=d_count.download(np.int32, (P + 1,)))
                for k in want:
                    assert np.array_equal(got[k], want[k]), (k, nxt, total, bank, rep)
            assert np.array_equal(d_mask.download(np.uint8, (n, m)), queue_mask)
    b.close()


# ---------------------------------------------------------------- 3. refusals
def test_refusals_write_nothing():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    L, n, m, P, total = nat.lib(), 2, 3, 4, 8
    b = ArenaBatch(n, m, width=W, height=H)
    assert L.ofx_restart_arenas(None, SEED, None) == nat.OFX_ERR_INVALID and L.ofx_last_error()
    assert L.ofx_restart_arenas(b.handle, SEED, None) == nat.OFX_ERR_STATE and b"ofx_spawn" in L.ofx_last_error()
    with pytest.raises(OfxError) as e:
        b.restart_arenas(SEED)
    assert e.value.code == nat.OFX_ERR_STATE
    with pytest.raises(OfxError):                                # nothing was allocated by the refused calls
        b.autoreset_state()
    b.spawn_random(SEED)
    member_of = np.array([[0, 1, P], [2, -1, 3]], np.int32)
    start = dict(member=member_of, mask=np.ones((n, m), np.uint8), queue=np.array([1, 0], np.int64),
                 sum=np.arange(P + 1, dtype=np.int64), count=np.ones(P + 1, np.int32))
    d = {k: _dev(v) for k, v in start.items()}
    args = lambda **kw: [kw.get("h", b.handle), kw.get("member", d["member"].ptr), kw.get("mask", d["mask"].ptr),
                         kw.get("P", P), kw.get("total", total), kw.get("queue", d["queue"].ptr),
                         kw.get("sum", d["sum"].ptr), kw.get("count", d["count"].ptr), 1]
    before = _state(b)
    # no per-arena episode state yet
    assert L.ofx_es_requeue(*args()) == nat.OFX_ERR_STATE and L.ofx_last_error()
    with pytest.raises(OfxError) as e:
        b.es_requeue(d["member"].ptr, d["mask"].ptr, P, total, d["queue"], d["sum"], d["count"])
    assert e.value.code == nat.OFX_ERR_STATE
    b.restart_arenas(SEED, _dev(np.zeros(n, np.uint8)))          # the state exists; no arena restarted
    after_restart = _state(b)
    assert _differences(before, after_restart) == []
    for kw in (dict(h=None), dict(member=None), dict(mask=None), dict(queue=None), dict(sum=None), dict(count=None),
               dict(P=5), dict(P=0), dict(P=-2), dict(P=1), dict(total=-1)):
        assert L.ofx_es_requeue(*args(**kw)) == nat.OFX_ERR_INVALID, kw
        assert L.ofx_last_error(), kw
    b.sync()
    for k, v in start.items():
        assert np.array_equal(d[k].download(v.dtype, v.shape), v), k
    assert _differences(after_restart, _state(b)) == []
    b.close()


# ---------------------------------------------------------------- 4. the loop against a host-side model
LOOP = dict(N=6, M=8, P=16, E=2, T=12, poll=4, sigma=0.05, lr=0.2, eval_arenas=1, generations=3)


def _host_queue_es():
    from ofighters_amd import _native as nat
    from ofighters_amd.es import ES

    class HostQueueES(ES):
        """ES whose requeue is the numpy law on downloaded arrays, uploaded again."""

        def requeue(self, bank=True):
            b, P = self.b, self.P
            restarted = b.autoreset_state()["restarted"]         # synchronises
            last = b.get(nat.F_LAST_SCORES)
            member = self._member_of.download(np.int32, (b.N, b.M))
            mask = self._queue_mask.download(np.uint8, (b.N, b.M))
            queue = self._queue.download(np.int64, (2,))
            s, c = self._sum.download(np.int64, (P + 1,)), self._count.download(np.int32, (P + 1,))
            qo.requeue(restarted, member, mask, last, P, self.queue_total, queue, s, c, int(bool(bank)))
            self._member_of.upload(member), self._queue.upload(queue), self._sum.upload(s), self._count.upload(c)

    return HostQueueES


def _rollout(cls, adaptive, init=True):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.es import ESRollout
    L = LOOP
    b = ArenaBatch(L["N"], L["M"], width=W, height=H)
    es = cls(b, [NIN, 9, 4], SEED, init=init, **(dict(sigma_init=L["sigma"]) if adaptive else {}))
    roll = ESRollout(b, es, ["random"] * L["M"], SEED, L["P"], None if adaptive else L["sigma"], L["lr"], ships=(0,),
                     eval_arenas=L["eval_arenas"], episode_ticks=L["T"], episodes_per_generation=L["E"],
                     auto_reset=True, poll_every=L["poll"])
    return b, es, roll


def _centre(es):
    return np.concatenate(es.b.es_get(es.n_weights, es.n_biases))


def _same_weights(x, y):
    return len(x) == len(y) and all(len(u) == len(v) and u[-1] == v[-1]
                                    and all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(u[:-1], v[:-1]))
                                    for u, v in zip(x, y))


def _loop(adaptive):
    """The device's loop and its twin on the numpy law, lock-step by lock-step through LOOP['generations'] generations.
    Returns what the device's run left."""
    from ofighters_amd.es import ES
    L = LOOP
    assert L["P"] > L["N"] * 1, "more members than arenas x evolved ships"
    (b1, es1, r1), (b2, es2, r2) = _rollout(ES, adaptive), _rollout(_host_queue_es(), adaptive)
    ends, members = [], []
    assert np.array_equal(es1.member_of_host(), es2.member_of_host()) and es1.queue_host() == es2.queue_host()
    assert es1.queue_host() == (L["N"] - L["eval_arenas"], 0)    # the begin handed a ticket to every learning arena
    while r1.generation < L["generations"]:
        assert r1.tick < 3000, "the generations do not end"
        g = r1.generation
        r1.lockstep(), r2.lockstep()
        m1, m2 = es1.member_of_host(), es2.member_of_host()
        assert np.array_equal(m1, m2), r1.tick
        assert es1.queue_host() == es2.queue_host(), r1.tick
        assert r1.generation == r2.generation
        members.append(m1)
        if r1.generation != g:
            ends.append(r1.tick - 1)                             # the lock-step whose head ended generation g
    assert np.array_equal(_bits(_centre(es1)), _bits(_centre(es2)))
    assert r1.fitness_log == r2.fitness_log and r1.centre_log == r2.centre_log
    assert r1.generation_log == r2.generation_log and _same_weights(r1.weight_log, r2.weight_log)
    s1, c1 = es1.fitness_host()
    s2, c2 = es2.fitness_host()
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2)
    out = dict(centre=_centre(es1), fitness_log=list(r1.fitness_log), centre_log=list(r1.centre_log),
               weight_log=list(r1.weight_log), generation_log=list(r1.generation_log), ends=ends, members=members,
               tick=r1.tick, score_log=list(r1.score_log), episode=b1.episode, member_of=es1.member_of_host(),
               arena_episode=b1.autoreset_state()["arena_episode"], sigmas=None)
    if adaptive:
        out["sigmas"] = np.concatenate(es1.b.es_sigma_get(es1.n_weights, es1.n_biases))
        assert np.array_equal(_bits(out["sigmas"]), _bits(np.concatenate(es2.b.es_sigma_get(es2.n_weights, es2.n_biases))))
    b1.close(), b2.close()
    return out


def _check_loop(r, adaptive):
    L = LOOP
    P, total = L["P"], L["P"] * L["E"]
    assert len(r["fitness_log"]) == len(r["centre_log"]) == len(r["weight_log"]) == len(r["generation_log"]) == 3
    # every generation flew EVERY member, E times: impossible with six arenas and one evolved ship without the queue
    assert all(w[-1] == P for w in r["weight_log"]), [w[-1] for w in r["weight_log"]]
    assert all(g[1] == total for g in r["generation_log"]) and all(g[2] > 0 for g in r["generation_log"])
    assert [e % L["poll"] for e in r["ends"]] == [0, 0, 0]
    assert [g[0] for g in r["generation_log"]] == list(np.diff([0] + r["ends"]))
    assert r["score_log"] == [] and r["episode"] == 0
    assert (r["arena_episode"] > 3).all()                        # every arena kept episodes of its own
    flown = np.stack(r["members"])[:, :L["N"] - 1, 0]
    assert set(np.unique(flown)) == set(range(-1, P)), "every member and the idle tail were seen in flight"
    assert (np.stack(r["members"])[:, L["N"] - 1, 0] == P).all() # the evaluation arena holds the centre throughout
    assert any(w[0].any() for w in r["weight_log"]), "no generation had an untied pair"
    print("generation_log:", r["generation_log"], "fitness_log:", r["fitness_log"], "centre_log:", r["centre_log"])


@pytest.fixture(scope="module")
def loop_run():
    return _loop(False)


def test_loop_against_the_host_side_model(loop_run):
    _check_loop(loop_run, False)


def test_loop_against_the_host_side_model_adaptive():
    r = _loop(True)
    _check_loop(r, True)
    assert r["sigmas"].min() < r["sigmas"].max(), "sigma never moved"


# ---------------------------------------------------------------- 5. resume
def test_loop_resumes_bit_for_bit(loop_run, tmp_path):
    from ofighters_amd.es import ES
    L, ref = LOOP, loop_run
    stop = ref["ends"][0] + L["T"] + 1                           # inside the second generation, between two polls, past
                                                                 # the lock-step at which the clock ended its first episodes
    assert stop % L["poll"] != 0 and stop < ref["ends"][1]
    b, es, roll = _rollout(ES, False)
    roll.run(stop)
    assert roll.generation == 1 and roll.tick == stop
    assert np.array_equal(es.member_of_host(), ref["members"][stop - 1])
    path = es.save(str(tmp_path / "centre.npy"))
    state = roll.state_dict()
    assert 0 < state["queue"][1] < state["queue"][0] <= L["P"] * L["E"], "stopped with evaluations in flight"
    b.close()
    b2, es2, roll2 = _rollout(ES, False, init=False)
    es2.load(path)
    roll2.load_state_dict(state)
    assert np.array_equal(es2.member_of_host(), ref["members"][stop - 1])
    roll2.run(ref["tick"] - stop)
    assert roll2.generation == L["generations"] and roll2.tick == ref["tick"]
    assert np.array_equal(_bits(_centre(es2)), _bits(ref["centre"]))
    assert roll2.fitness_log == ref["fitness_log"] and roll2.centre_log == ref["centre_log"]
    assert roll2.generation_log == ref["generation_log"] and _same_weights(roll2.weight_log, ref["weight_log"])
    assert np.array_equal(es2.member_of_host(), ref["member_of"])
    assert np.array_equal(b2.autoreset_state()["arena_episode"], ref["arena_episode"])
    b2.close()
