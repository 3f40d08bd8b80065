"""Packed frame store, the part that needs no GPU: the numpy model of the storing rule on hand-made counts, the
argument checks of DeviceTrainer / ArenaBatch.replay_create against a stand-in batch, and the two new C-ABI entry points
in the header, the library and the binding (tests/test_abi.py then checks that the three agree on every symbol)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ofighters_amd import _native as nat
from tests.packed_ring_model import PackedRing, eligible

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------ the model
def test_model_stores_without_eviction_while_the_pool_holds_the_ring():
    r = PackedRing(frames=4, pool_pairs=100)
    for t, k in enumerate([(10, 5), (0, 0), (20, 1), (3, 3)]):
        r.store(t, *k)
    assert r.live_ticks() == [0, 1, 2, 3] and r.live == 42 and r.evicted == 0 and r.pool_head == 42
    assert list(r.off) == [0, 15, 15, 36]
    r.store(4, 30, 0)                                 # the slot ring wraps: frame 0 leaves by step 1, not an eviction
    assert r.live_ticks() == [1, 2, 3, 4] and r.live == 42 - 15 + 30 and r.evicted == 0
    assert r.off[0] == 42 and r.pool_head == 72 and r.frame_head == 1


def test_model_evicts_oldest_first_and_wraps_the_pool():
    r = PackedRing(frames=5, pool_pairs=40)
    r.store(0, 10, 2)
    r.store(1, 8, 0)
    r.store(2, 9, 1)                                  # live 30
    r.store(3, 15, 0)                                 # 45 > 40: frame 0 goes (33)
    assert r.live_ticks() == [1, 2, 3] and r.evicted == 1 and r.live == 33
    assert r.frame_tick[0] == -1 and r.cnt[0].sum() == 0
    assert r.off[3] == 30 and r.pool_head == 5        # its pairs wrap: 30 .. 39, 0 .. 4
    r.store(4, 20, 0)                                 # 53 > 40: frames 1 (45) and 2 (35) go
    assert r.live_ticks() == [3, 4] and r.evicted == 3 and r.live == 35 and r.pool_head == 25
    r.store(5, 0, 0)                                  # slot 0 again: it holds no live frame, step 1 releases nothing
    assert r.live_ticks() == [3, 4, 5] and r.live == 35 and r.evicted == 3
    # live ranges never overlap, and they are a cyclic run that ends at pool_head
    rg = r.ranges()
    assert sum(len(v) for v in rg.values()) == len(set().union(*rg.values())) == r.live
    assert set().union(*rg.values()) == {(r.pool_head - 1 - i) % r.pool for i in range(r.live)}


def test_model_random_runs_keep_the_invariants_and_repack_alike():
    rs = np.random.RandomState(5)
    for frames, pool in ((3, 40), (7, 64), (22, 200)):
        r = PackedRing(frames, pool)
        stored = []
        for t in range(300):
            if rs.rand() < 0.2:
                continue                              # a lock-step on which nothing plays stores nothing
            r.store(t, int(rs.randint(0, pool // 4 + 1)), int(rs.randint(0, pool // 4 + 1)))
            stored.append(t)
            live = r.live_ticks()
            assert live == stored[-len(live):] and 1 <= len(live) <= frames     # the newest ones, never none
            assert r.live == int(r.cnt.sum()) <= pool
            rg = r.ranges()
            assert sum(len(v) for v in rg.values()) == r.live == len(set().union(*rg.values()))
            if t % 50 == 49:                          # the import's placement behaves identically from then on
                q, twin = r.repacked(), PackedRing(frames, pool)
                assert q is not None and q.live == r.live and q.pool_head == r.live % pool
                twin.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.__dict__.items()})
                for u in range(t + 1, t + 30):
                    k = (int(rs.randint(0, pool // 4 + 1)), int(rs.randint(0, pool // 4 + 1)))
                    q.store(u, *k), twin.store(u, *k)
                    assert q.live_ticks() == twin.live_ticks() and q.live == twin.live
                assert q.evicted == twin.evicted - r.evicted
        assert r.evicted > 0


def test_model_repack_refuses_a_smaller_pool():
    r = PackedRing(4, 100)
    for t in range(4):
        r.store(t, 20, 0)
    small = PackedRing(4, 60)
    small.frame_tick, small.cnt, small.frame_head = r.frame_tick.copy(), r.cnt.copy(), r.frame_head
    assert small.repacked() is None and r.repacked().live == 80


def test_model_eligible_rows():
    rows = np.zeros(4, [("tick_prev", np.int32), ("frame_prev", np.int32)])
    rows["tick_prev"], rows["frame_prev"] = [3, 4, 5, 6], [0, 1, 2, 0]
    assert eligible(rows, np.array([6, 4, 5])) == 3   # row 0's slot holds lock-step 6 now
    assert eligible(rows, np.array([6, -1, -1])) == 1
    assert eligible(rows, np.array([-1, -1, -1])) == 0 and eligible(rows[:0], np.array([1])) == 0


# ------------------------------------------------------------------------------------------------ argument checks
class _StandIn:
    """An ArenaBatch that must never be asked for anything: the checks come before the first allocation."""
    N = M = 1

    def __getattr__(self, name):
        raise AssertionError("the batch was touched (%s) before the arguments were checked" % name)


@pytest.mark.parametrize("kw", [dict(packed_memory=True, memory_pool_pairs=-1), dict(packed_memory=True, memory_pool_pairs=2.0),
                                dict(packed_memory=True, memory_pool_pairs=True), dict(packed_memory=True, memory_pool_pairs="9"),
                                dict(packed_memory=False, memory_pool_pairs=20000)])
def test_trainer_refuses_bad_pool_arguments_before_allocating(kw):
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match="memory_pool_pairs"):
        DeviceTrainer(_StandIn(), np.zeros(4, np.float32), **kw)


@pytest.mark.parametrize("kw", [dict(packed=True, pool_pairs=-5), dict(packed=True, pool_pairs=1.5),
                                dict(packed=True, pool_pairs=False), dict(packed=False, pool_pairs=4096)])
def test_replay_create_refuses_bad_pool_arguments(kw):
    from ofighters_amd import ArenaBatch
    with pytest.raises(ValueError, match="pool_pairs"):
        ArenaBatch.replay_create(_StandIn(), 16, 0, **kw)


def test_pool_arguments_stay_out_of_the_fingerprint():
    from ofighters_amd.trainer import DeviceTrainer
    t = object.__new__(DeviceTrainer)
    for k in ("n_floats", "learning_rate", "gamma", "batch_size", "fit_batch", "seed", "per_alpha", "per_beta", "per_beta_steps",
              "per_eps", "n_step", "target_sync"):
        setattr(t, k, 1)
    t.reference_quirks = t.prioritized = t.double_dqn = False
    t.target_tau = t.huber_delta = t.clip_norm = None
    t.packed_memory, t.memory_pool_pairs = True, 20000

    class B:
        replay_capacity, replay_frames = 16, 22
    t.batch = B()
    assert not any("pool" in k or "packed" in k for k in t.fingerprint())


# ------------------------------------------------------------------------------------------------------- the ABI
def test_packed_entry_points_are_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ofx.h")).read(), flags=re.S)
    L = C.CDLL(nat.LIB_PATH)
    for name, nargs in (("ofx_replay_create_packed", 4), ("ofx_replay_store_stats", 2)):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), "%s is not declared in include/ofx.h" % name
        assert hasattr(L, name), "libofx.so does not export %s" % name
        assert len(nat.SIGNATURES[name][1]) == nargs
    assert nat.SIGNATURES["ofx_replay_create_packed"][1][3] is C.c_int64


def test_packed_entry_points_fail_loudly_without_a_handle():
    L = nat.lib()
    assert L.ofx_replay_create_packed(None, 16, 0, 0) == nat.OFX_ERR_INVALID
    v = (C.c_int64 * 6)()
    assert L.ofx_replay_store_stats(None, v) == nat.OFX_ERR_INVALID
