"""Checkpoints on the device: the replay memory's export / import (the pack and scatter kernels of ofx_replay.hip)
against the host inspections and tests/ckpt_blob.py, and a TrainingRollout stopped, written to disk, restored into fresh
handles and continued - bit-identical to the run that never stopped."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import ckpt_blob
from tests.train_state import check_decoded as _check_decoded, inspect_replay as _inspect, training_state as _state

pytestmark = pytest.mark.gpu

W = H = 400
WORDS = W * H // 32


# ------------------------------------------------------------------------------------------ 1. the replay memory
N1, M1, CAP = 5, 8, 8                       # 5 arenas: four share a block of the pack kernels, the last block is partial
SEED1 = 0x0F160021
MASKED = (2, 3, 4)                          # the capturing ships
BEHAVIOURS = ["idle", "idle"] + ["random"] * 6
ALPHA, EPS = 0.6, 1e-3


def _positions(seed):
    """Ship 0 at (0, 0) and ship 1 at (W-1, H-1) - their discs set the first and the last word of a map -, the others
    packed into the box of the golden brawl traces, where random bots shoot each other."""
    rs = np.random.RandomState(seed & 0xFFFF)
    x, y = rs.randint(150, 250, (N1, M1)), rs.randint(150, 250, (N1, M1))
    x[:, 0] = y[:, 0] = 0
    x[:, 1], y[:, 1] = W - 1, H - 1
    return x.astype(np.int32), y.astype(np.int32)


class _Scenario:
    """The scripted run of test 1 on one handle; step(t) is a pure function of (handle state, t)."""

    def __init__(self, b):
        from ofighters_amd import DeviceBuffer
        self.b = b
        mk = np.zeros((N1, M1), np.uint8)
        mk[:, list(MASKED)] = 1
        self.mask = DeviceBuffer(mk.nbytes).upload(mk)
        self.ia, self.ip = DeviceBuffer(4 * N1 * M1), DeviceBuffer(8 * N1 * M1)

    def place(self):
        x, y = _positions(SEED1)
        self.b.set_ships(x=x, y=y)

    def step(self, t, churn=False):
        b = self.b
        if churn:                           # arena 1 starts an episode on every lock-step: frames without rows
            x, y = _positions(SEED1 + t)
            b.restart(np.stack([x, y], -1), arena_mask=np.arange(N1) == 1)
        rs = np.random.RandomState(1000 + t)
        ia = rs.randint(0, 2, (N1, M1)).astype(np.int32)
        ip = np.stack([rs.randint(0, W, (N1, M1)), rs.randint(0, H, (N1, M1))], -1).astype(np.int32)
        b.sync()
        self.ia.upload(ia), self.ip.upload(ip)
        b.bot_actions(BEHAVIOURS, SEED1, tick=t)
        b.replay_capture(t, self.mask.ptr, self.ia.ptr, self.ip.ptr)
        b.step()

    def reprioritize(self, t):
        """replay_update_priorities over every row of every arena with TD errors that depend on the row."""
        from ofighters_amd import DeviceBuffer, _native as nat
        b = self.b
        cnt, _ = b.replay_count()
        slot = np.full((N1, CAP), -1, np.int32)
        for a in range(N1):
            slot[a, :cnt[a]] = np.arange(cnt[a])
        total = int(cnt.sum())
        slot_d, n_d = DeviceBuffer(slot.nbytes).upload(slot), DeviceBuffer(4 * N1).upload(cnt.astype(np.int32))
        rows, n = DeviceBuffer(max(1, total) * b.TRANSITION_DTYPE.itemsize), C.c_int32()
        nat.check(nat.lib().ofx_replay_gather_valid(b.handle, slot_d.ptr, n_d.ptr, CAP, 0, total, rows.ptr, None, None,
                                                     C.byref(n)))
        assert n.value == total
        r = rows.download(b.TRANSITION_DTYPE, (total,))
        td = np.stack([0.01 * (r["tick_prev"] + t) + 0.1 * r["ship"], 0.5 * r["iaction"] + 0.001 * r["px"]], 1).astype(np.float32)
        b.replay_update_priorities(slot_d, n_d, CAP, 0, total, rows.ptr, DeviceBuffer(td.nbytes).upload(td).ptr)
        b.sync()


def _fresh():
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N1, M1)
    b.spawn_random(SEED1)
    b.replay_create(capacity=CAP, frames=0)
    b.replay_prioritize(ALPHA, EPS)
    return b


def _same(x, y):
    return (np.array_equal(x["count"], y["count"]) and np.array_equal(x["appended"], y["appended"]) and x["rows"] == y["rows"]
            and x["mass"] == y["mass"] and x["frames"] == y["frames"])


def _samples(b, draw):
    slot, n = b.replay_sample(SEED1, draw, 4)
    pslot, pn, piw = b.replay_sample_prioritized(SEED1, draw, 4, 0.4)
    b.sync()
    return (slot.download(np.int32, (b.N, 4)).tobytes(), n.download(np.int32, (b.N,)).tobytes(),
            pslot.download(np.int32, (b.N, 4)).tobytes(), pn.download(np.int32, (b.N,)).tobytes(),
            piw.download(np.float32, (b.N, 4)).tobytes())


def test_replay_memory_round_trips_through_its_blob():
    """30 lock-steps of a brawl with a restart after 15, captures for three ships with explicit actions, priorities
    rewritten on the way.  With one episode start per 15 lock-steps a frame ring of C + C / 4 + 2 slots can never lose a
    frame that a live row needs (frames stored minus rows appended is at most the number of episode starts), so arena 1
    additionally starts an episode on every lock-step from 16 on: its ring fills with frames that carry no row and all
    its rows lose their `state` frame."""
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    a = _fresh()
    sa = _Scenario(a)
    sa.place()
    for t in range(30):
        if t == 15:
            a.restart_random(SEED1)
            sa.place()
        sa.step(t, churn=t >= 16)
        if t in (6, 13, 22, 27):
            sa.reprioritize(t)
    a.sync()
    T = 30
    ins = _inspect(a, T)
    # ---- the preconditions of this test, asserted so that they cannot quietly stop holding
    assert ins["appended"].max() > CAP                                   # rows were overwritten
    expired = [x for x in range(N1) if ins["count"][x] and int(a.replay_rows(x)["tick_prev"][0]) not in ins["frames"][x]]
    assert expired, "no arena's oldest row has lost its frame"
    alive = a.get(nat.F_SHIP_ALIVE)
    assert (alive[:, list(MASKED)] == 0).any(), "no capturing ship is dead at the export"
    empty = np.packbits(np.zeros((H, W), np.uint8)).tobytes()
    assert any(f[1] == empty for held in ins["frames"] for f in held.values()), "no stored laser map is empty"
    # ---- export: chunks [0, 3) and [3, 5)
    chunks = [(0, 3), (3, 2)]
    blobs = [a.replay_export(a0, n) for a0, n in chunks]
    assert [a.replay_export_bytes(a0, n) for a0, n in chunks] == [b.nbytes for b in blobs]
    assert all(np.array_equal(a.replay_export(a0, n), b) for (a0, n), b in zip(chunks, blobs))   # byte-identical again
    decs = [ckpt_blob.decode(b) for b in blobs]
    for (a0, n), d, blob in zip(chunks, decs, blobs):
        assert (d["W"], d["H"], d["M"], d["C"], d["F"], d["n"], d["per"]) == (W, H, M1, CAP, CAP + CAP // 4 + 2, n, 1)
        assert (np.float32(d["alpha"]), np.float32(d["eps"])) == (np.float32(ALPHA), np.float32(EPS))
        _check_decoded(d, ins, a0)
        assert ckpt_blob.encode(d) == blob.tobytes()                     # the layout text alone gives the same bytes
    maps = np.concatenate([d["maps"] for d in decs])
    assert ((maps[:, :, 0, 0] != 0) & (maps[:, :, 0, WORDS - 1] != 0)).any(), "no stored map has its first and last word set"
    latched = np.concatenate([d["latched"] for d in decs])
    assert latched[:, list(MASKED)].any() and not latched[:, [0, 1, 5, 6, 7]].any()
    # ---- a destination one byte short: refused, untouched
    need = blobs[1].nbytes
    dst, wrote = np.full(need, 0xAB, np.uint8), C.c_size_t(77)
    rc = nat.lib().ofx_replay_export(a.handle, 3, 2, dst.ctypes.data_as(C.c_void_p), need - 1, C.byref(wrote))
    assert rc == nat.OFX_ERR_INVALID and (dst == 0xAB).all() and wrote.value == 77
    # ---- import into a fresh handle
    b = _fresh()
    b.load_state_dict(a.state_dict())
    for (a0, n), blob in zip(chunks, blobs):
        b.replay_import(a0, n, blob)
    assert _same(_inspect(b, T), ins)
    assert all(np.array_equal(b.replay_export(a0, n), blob) for (a0, n), blob in zip(chunks, blobs))
    sd_a, sd_b = a.state_dict(), b.state_dict()
    assert all(np.array_equal(sd_a[k], sd_b[k]) for k in sd_a)
    # ---- both continue alike
    sb = _Scenario(b)
    for t in range(T, T + 10):
        for s in (sa, sb):
            s.step(t)
            if t == T + 4:
                s.reprioritize(t)
    a.sync(), b.sync()
    ins_a, ins_b = _inspect(a, T + 10), _inspect(b, T + 10)
    assert _same(ins_a, ins_b) and not _same(ins_a, ins)
    assert all(_samples(a, d) == _samples(b, d) for d in (0, 1, 9))
    # ---- a handle of another shape refuses the blob and stays as it was
    for cap, per in ((9, True), (CAP, False)):
        c = ArenaBatch(N1, M1)
        c.spawn_random(SEED1)
        c.replay_create(capacity=cap, frames=0)
        if per:
            c.replay_prioritize(ALPHA, EPS)
        sc = _Scenario(c)
        for t in range(3):
            sc.step(t)
        c.sync()
        look = lambda: (c.replay_count()[0].tobytes(), [c.replay_rows(x).tobytes() for x in range(N1)],
                        [c.replay_frame(x, 1)[0].tobytes() for x in range(N1)])
        before = look()
        with pytest.raises(OfxError) as err:
            c.replay_import(0, 3, blobs[0])
        assert ("capacity" if cap == 9 else "prioritized") in str(err.value)
        assert look() == before
        c.close()
    # ---- a blob the device never produced
    d = ckpt_blob.decode(blobs[1])
    rs = np.random.RandomState(3)
    slot = int(np.flatnonzero(d["frame_tick"][1] >= 0)[0])
    d["maps"][1, slot, 1] = rs.randint(1, 2**31, WORDS).astype(np.uint32)        # every word of one map nonzero
    d["maps"][0] = np.roll(d["maps"][0], 7, axis=-1)
    d["mass"] = (d["mass"] * 0.5 + 0.125).astype(np.float32)
    d["mmax"] = (d["mmax"] + 1).astype(np.float32)
    rows = d["rows"]
    rows["reward"] += 3
    made = ckpt_blob.encode(d)
    b.replay_import(3, 2, np.frombuffer(made, np.uint8))
    ins_m = _inspect(b, T + 10)
    _check_decoded(d, ins_m, 3)
    assert b.replay_export(3, 2).tobytes() == made
    assert ins_m["rows"][:3] == ins_b["rows"][:3] and ins_m["frames"][:3] == ins_b["frames"][:3]   # the other chunk: untouched
    a.close(), b.close()


# ------------------------------------------------------------------------------------- 2. resume is bit-identical
N2, M2, SEED2 = 6, 4, 0x0F160023
CONFIGS = {"defaults": {},
           "everything": dict(prioritized=True, n_step=3, target_sync=2, double_dqn=True, huber_delta=1.0, clip_norm=10.0)}
TOTAL = 50


def _build(cfg, **roll_kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N2, M2)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=16,
                       **CONFIGS[cfg])
    roll = TrainingRollout(b, tr, ["random"] * M2, SEED2, policy_ships=(0, 1), episode_ticks=20, collecting_steps=5,
                           replay_every=3, **roll_kw)
    return b, tr, roll


_RUN_A = {}


def _run_a(cfg):
    """The run that never stops, once per configuration: its state after every split and at the end."""
    if cfg not in _RUN_A:
        b, tr, roll = _build(cfg)
        out = {}
        for stop in (20, 25, TOTAL):
            roll.run(stop - roll.tick)
            out[stop] = _state(b, tr, roll)
        b.close()
        _RUN_A[cfg] = out
    return _RUN_A[cfg]


@pytest.mark.parametrize("split", [25, 20])          # mid-episode / on the boundary: the restart is the next thing done
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_resume_is_bit_identical(tmp_path, cfg, split):
    ref = _run_a(cfg)
    b, tr, roll = _build(cfg)
    roll.run(split)
    assert tr.fit_steps >= 3 and ref[TOTAL]["fit_steps"] >= tr.fit_steps + 3
    if CONFIGS[cfg].get("prioritized"):
        assert any(len(set(b.replay_priorities(a).tolist())) > 1 for a in range(N2)), "every priority is still equal"
    assert _state(b, tr, roll) == ref[split]
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    b.close()
    del b, tr, roll
    b, tr, roll = _build(cfg)
    m = roll.restore(path)
    assert m["counters"]["tick"] == split
    after = _state(b, tr, roll)
    assert [k for k in after if after[k] != ref[split][k]] == []
    roll.run(TOTAL - split)
    end = _state(b, tr, roll)
    assert [k for k in end if end[k] != ref[TOTAL][k]] == []      # names what differs; every entry is compared with ==
    assert end == ref[TOTAL]
    b.close()


def test_restore_refuses_a_differently_built_run(tmp_path):
    b, tr, roll = _build("everything")
    roll.run(8)
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    b.close()
    b, tr, roll = _build("defaults")
    roll.run(3)
    before = _state(b, tr, roll)
    with pytest.raises(ValueError) as err:
        roll.restore(path)
    for key in ("prioritized", "n_step", "target_sync", "double_dqn", "huber_delta", "clip_norm"):
        assert "trainer.%s " % key in str(err.value)
    assert _state(b, tr, roll) == before
    b.close()


# ------------------------------------------------------------------------------------------- 3. checkpoint_every
def test_checkpoint_every_episode(tmp_path):
    folder = str(tmp_path / "auto")
    b, tr, roll = _build("defaults", checkpoint_every=1, checkpoint_folder=folder)
    latest = os.path.join(folder, "checkpoint-latest")
    seen = []
    for ep in range(3):
        roll.run(19)
        assert (not os.path.exists(folder)) if ep == 0 else open(latest, "rb").read() == seen[-1]
        roll.run(1)                                   # the lock-step that completes the episode writes the checkpoint
        assert os.listdir(folder) == ["checkpoint-latest"]
        seen.append(open(latest, "rb").read())
        manual = str(tmp_path / ("manual%d" % ep))
        roll.checkpoint(manual)
        assert open(manual, "rb").read() == seen[-1]
    assert len(set(seen)) == 3
    here = _state(b, tr, roll)
    b.close()
    b, tr, roll = _build("defaults", checkpoint_every=1, checkpoint_folder=folder)
    roll.restore(latest)
    assert _state(b, tr, roll) == here
    b.close()
