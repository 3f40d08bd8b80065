"""Packed frame store on the device (include/ofx.h, "packed frame store"): a packed memory driven in lock-step with a
dense twin returns the same bytes from every reader, exports the same blob and crosses forms through it; a pool that is
too small evicts early exactly as tests/packed_ring_model.py predicts from the dense twin's frames; and a DeviceTrainer
on a packed memory fits the same bits.  Everything is compared with ==."""
import ctypes as C

import numpy as np
import pytest

from tests.packed_ring_model import PackedRing, eligible

pytestmark = pytest.mark.gpu

N, M, CAP, FRAMES = 5, 3, 17, 22            # 5 arenas: the capture kernel takes 4 per workgroup, the last block is partial
SEED = 0x0F160031
MASKED = (0, 1)                             # the capturing ships
ALPHA, EPS = 0.6, 1e-3
DEAD = ((2, 0), (3, 0), (3, 1))             # (arena, ship) dead from every episode start: arena 3 stops playing at once


def _nonzero_words(m):
    """Nonzero 32-bit words of a map given as uint8 [H][W] pixels."""
    return int(m.reshape(-1, 32).any(axis=1).sum())


class _Twin:
    """One handle of a pair that is driven identically; step(t) is a pure function of (handle state, t)."""

    def __init__(self, packed, pool_pairs=0, per=True, behaviours=None, n_ships=M, masked=MASKED, dead=DEAD, **cfg):
        from ofighters_amd import ArenaBatch, DeviceBuffer
        self.M, self.dead = n_ships, dead
        self.b = b = ArenaBatch(N, n_ships, **cfg)
        self.behaviours = behaviours or ["random", "random", "idle"]
        b.spawn_random(SEED)
        b.replay_create(CAP, FRAMES, packed=packed, pool_pairs=pool_pairs)
        if per:
            b.replay_prioritize(ALPHA, EPS)
        mk = np.zeros((N, n_ships), np.uint8)
        mk[:, list(masked)] = 1
        self.mask = DeviceBuffer(mk.nbytes).upload(mk)
        self.ia, self.ip = DeviceBuffer(4 * N * n_ships), DeviceBuffer(8 * N * n_ships)
        self.kill()

    def kill(self):
        d = self.b.state_dict()
        for a, s in self.dead:
            d["ship_alive"][a, s] = 0
        self.b.load_state_dict(d)

    def step(self, t, restart_every=25):
        b = self.b
        if t and restart_every and t % restart_every == 0:
            b.restart_random(SEED)
            self.kill()
        rs = np.random.RandomState(2000 + t)
        ia = rs.randint(0, 2, (N, self.M)).astype(np.int32)
        ip = np.stack([rs.randint(0, b.W, (N, self.M)), rs.randint(0, b.H, (N, self.M))], -1).astype(np.int32)
        b.sync()
        self.ia.upload(ia), self.ip.upload(ip)
        b.bot_actions(self.behaviours, SEED, tick=t)
        b.replay_capture(t, self.mask.ptr, self.ia.ptr, self.ip.ptr)
        b.step()


def _frames(b, ticks):
    """Per arena {tick: (ship map, laser map) packed bytes} of the held frames; an absent tick must be OFX_ERR_STATE."""
    from ofighters_amd import OfxError, _native as nat
    out = []
    for a in range(b.N):
        held = {}
        for t in range(ticks):
            try:
                s, l = b.replay_frame(a, t)
                held[t] = (np.packbits(s).tobytes(), np.packbits(l).tobytes())
            except OfxError as e:
                assert e.code == nat.OFX_ERR_STATE
        out.append(held)
    return out


def _dl(buf, dtype, shape):
    return buf.download(dtype, shape).tobytes()


def _gathers(b, draw, per=True):
    """Everything the samplers and the gathers return for one draw, as bytes (per: and one priority write-back)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    words = b.W * b.H // 32
    out = {}
    for batch in (4, 32):                                    # 32 is above some arenas' counts
        slot, n = b.replay_sample(SEED, draw, batch)
        b.sync()
        out["slot%d" % batch], out["n%d" % batch] = _dl(slot, np.int32, (N, batch)), _dl(n, np.int32, (N,))
        rows, bp, bn = b.replay_gather(slot, batch)
        s = slot.download(np.int32, (N, batch))
        assert (s < 0).any() or batch == 4
        assert not bp[s < 0].any() and not bn[s < 0].any() and (rows["ship"][s < 0] == -1).all()   # the pads: empty maps
        out["gather%d" % batch] = (rows.tobytes(), bp.tobytes(), bn.tobytes())
        n_valid = int(n.download(np.int32, (N,)).sum())
        first, max_rows = 3, min(10, n_valid - 3)            # a window that starts inside arena 0 and cuts a later one
        assert max_rows > 0
        r2, p2, q2, got = b.replay_gather_valid(slot, n, batch, first, max_rows)
        b.sync()
        out["valid%d" % batch] = (got, _dl(r2, b.TRANSITION_DTYPE, (got,)), _dl(p2, np.uint32, (got, 2, words)),
                                  _dl(q2, np.uint32, (got, 2, words)))
        rows_d = DeviceBuffer(max_rows * b.TRANSITION_DTYPE.itemsize)
        bp_d, bn_d = DeviceBuffer(8 * max_rows * words), DeviceBuffer(8 * max_rows * words)
        ret, disc = DeviceBuffer(4 * max_rows), DeviceBuffer(4 * max_rows)
        got = b.replay_gather_nstep_into(slot, n, batch, first, max_rows, 3, 0.9, rows_d, bp_d, bn_d, ret, disc)
        b.sync()
        out["nstep%d" % batch] = (got, _dl(rows_d, b.TRANSITION_DTYPE, (got,)), _dl(bp_d, np.uint32, (got, 2, words)),
                                  _dl(bn_d, np.uint32, (got, 2, words)), _dl(ret, np.float32, (got,)), _dl(disc, np.float32, (got,)))
    if per and b.replay_prioritized:
        slot, n, isw = b.replay_sample_prioritized(SEED, draw, 4, 0.4)
        b.sync()
        out["per"] = (_dl(slot, np.int32, (N, 4)), _dl(n, np.int32, (N,)), _dl(isw, np.float32, (N, 4)))
        n_valid = int(n.download(np.int32, (N,)).sum())
        rows_d = DeviceBuffer(n_valid * b.TRANSITION_DTYPE.itemsize)
        got = C.c_int32()
        nat.check(nat.lib().ofx_replay_gather_valid(b.handle, slot.ptr, n.ptr, 4, 0, n_valid, rows_d.ptr, None, None, C.byref(got)))
        r = rows_d.download(b.TRANSITION_DTYPE, (n_valid,))
        td = np.stack([0.01 * (r["tick_prev"] + draw) + 0.1 * r["ship"], 0.5 * r["iaction"] + 0.001 * r["px"]], 1).astype(np.float32)
        td_d = DeviceBuffer(td.nbytes).upload(td)
        b.replay_update_priorities(slot, n, 4, 0, n_valid, rows_d.ptr, td_d.ptr)
        b.sync()
        out["mass"] = [b.replay_priorities(a).tobytes() for a in range(N)]
    return out


def _look(b, ticks, draw, gathers=True):
    cnt, app = b.replay_count()
    out = {"count": cnt.tobytes(), "appended": app.tobytes(), "rows": [b.replay_rows(a).tobytes() for a in range(N)],
           "frames": _frames(b, ticks)}
    if gathers:
        out.update(_gathers(b, draw))
    return out


def _differing(x, y):
    return [k for k in sorted(set(x) | set(y)) if x.get(k) != y.get(k)]


def _store_bytes(pool_pairs, frames=FRAMES, n=N):
    return n * (pool_pairs * 8 + frames * 4 + frames * 2 * 4 + 4 + 4 + 8)       # section 1 of the contract


# ---------------------------------------------------------------------------------- 1 + 2. packed == dense, the blob
T_RUN, T_MID = 70, 40
BIG = dict(ship_radius=40)                  # discs of about 240 words: 22 live frames stay inside the pool, 70 wrap it
_PAIR = {}


def _pair():
    """The 70 lock-steps of tests 1 and 2 on a dense and a packed handle, once: the handles, the mid-run looks and the
    per-frame pair counts of the dense twin."""
    if not _PAIR:
        words = 400 * 400 // 32
        d, p = _Twin(False, **BIG), _Twin(True, 4 * words, **BIG)
        counts = [dict() for _ in range(N)]
        mid = None
        for t in range(T_RUN):
            d.step(t), p.step(t)
            for a in range(N):
                try:
                    s, l = d.b.replay_frame(a, t)
                    counts[a][t] = (_nonzero_words(s), _nonzero_words(l))
                except Exception:
                    pass                                     # nothing played in this arena on this lock-step
            if t == T_MID - 1:
                mid = (_look(d.b, T_MID, 5), _look(p.b, T_MID, 5), p.b.replay_store_stats())
        _PAIR.update(d=d, p=p, counts=counts, mid=mid, words=words)
    return _PAIR


def test_packed_equals_dense():
    z = _pair()
    d, p, counts, words = z["d"].b, z["p"].b, z["counts"], z["words"]
    pool = 4 * words
    assert _differing(z["mid"][0], z["mid"][1]) == [] and z["mid"][2]["evicted"] == 0
    ld, lp = _look(d, T_RUN, 9), _look(p, T_RUN, 9)
    assert _differing(ld, lp) == []
    # ---- the preconditions, asserted so that they cannot quietly stop holding
    cnt, app = d.replay_count()
    stored = [len(c) for c in counts]
    totals = [sum(a + b for a, b in c.values()) for c in counts]
    print("frames stored", stored, "pairs stored", totals, "pool", pool, "stats", p.replay_store_stats())
    assert max(stored) > FRAMES and app.max() > CAP                      # the slot ring and the row ring wrapped
    assert min(stored) < T_RUN // 2                                      # an arena with lock-steps on which nothing plays
    assert sum(1 for x in totals if x > pool) >= 2                       # the pool wrapped in at least two arenas
    assert min(sum(c) for cs in counts for c in cs.values()) < 300       # frames with few pairs
    assert any(len(h) < len(c) for h, c in zip(ld["frames"], counts))    # absent ticks were compared too
    # ---- the store's own numbers
    sd, sp = d.replay_store_stats(), p.replay_store_stats()
    assert sd == {"packed": 0, "pool_pairs": 0, "live_max": 0, "live_sum": 0, "evicted": 0,
                  "store_bytes": 4 * N * FRAMES * 2 * words}
    live = [sum(sum(counts[a][t]) for t in ld["frames"][a]) for a in range(N)]
    assert sp == {"packed": 1, "pool_pairs": pool, "live_max": max(live), "live_sum": sum(live), "evicted": 0,
                  "store_bytes": _store_bytes(pool)}


def _subset(b, ticks):
    return _look(b, ticks, 0, gathers=False), _gathers(b, 3, per=False)["gather4"]


def test_packed_export_is_byte_identical_and_crosses_forms():
    z = _pair()
    d, p, words = z["d"].b, z["p"].b, z["words"]
    blobs_d = [d.replay_export(0, 5), d.replay_export(1, 3)]
    blobs_p = [p.replay_export(0, 5), p.replay_export(1, 3)]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(blobs_d, blobs_p))
    assert [p.replay_export_bytes(0, 5), p.replay_export_bytes(1, 3)] == [x.nbytes for x in blobs_d]
    want = _subset(d, T_RUN)
    # the dense blob into a fresh packed handle, the packed blob into a fresh dense one
    q, e = _Twin(True, 4 * words, **BIG), _Twin(False, **BIG)
    for fresh, blob in ((q, blobs_d[0]), (e, blobs_p[0])):
        fresh.b.load_state_dict(d.state_dict())
        fresh.b.replay_import(0, 5, blob)
        got = _subset(fresh.b, T_RUN)
        assert _differing(got[0], want[0]) == [] and got[1] == want[1]
        assert fresh.b.replay_export(0, 5).tobytes() == blob.tobytes()
    sq = q.b.replay_store_stats()
    assert (sq["live_sum"], sq["live_max"], sq["evicted"]) == (p.replay_store_stats()["live_sum"], p.replay_store_stats()["live_max"], 0)
    # twenty further lock-steps: 20 frames could need 10 * words pairs, the re-packed pool of 4 * words wraps again
    for t in range(T_RUN, T_RUN + 20):
        q.step(t), e.step(t)
    lq, le = _look(q.b, T_RUN + 20, 11), _look(e.b, T_RUN + 20, 11)
    assert _differing(lq, le) == [] and lq["rows"] != want[0]["rows"]
    assert q.b.replay_export(0, 5).tobytes() == e.b.replay_export(0, 5).tobytes()
    assert q.b.replay_store_stats()["evicted"] == 0
    q.b.close(), e.b.close()


def test_packed_create_checks_its_pool():
    from ofighters_amd import ArenaBatch, OfxError, _native as nat
    b = ArenaBatch(2, 2)
    b.spawn_random(1)
    with pytest.raises(OfxError, match="no replay memory") as err:
        b.replay_store_stats()
    assert err.value.code == nat.OFX_ERR_STATE
    for bad in (1, 4 * 5000 - 1, 2**31):
        with pytest.raises(OfxError, match=r"\[20000, 2147483648\)") as err:
            b.replay_create(8, 0, packed=True, pool_pairs=bad)
        assert err.value.code == nat.OFX_ERR_INVALID
    b.replay_create(8, 0, packed=True)                                   # the default: max(512 * 12, 4 * words)
    assert b.replay_store_stats() == {"packed": 1, "pool_pairs": 20000, "live_max": 0, "live_sum": 0, "evicted": 0,
                                      "store_bytes": _store_bytes(20000, 12, 2)}
    b.replay_create(400, 0, packed=True)
    assert b.replay_store_stats()["pool_pairs"] == 512 * 502
    b.close()


# ------------------------------------------------------------------------------------------------ 3. early eviction
SMALL = dict(width=128, height=128)         # words = 512: the minimum pool is 2048 pairs, a frame of 8 ships near 250
M3 = 8
T3 = 40


def test_early_eviction_follows_the_rule():
    from ofighters_amd import OfxError, _native as nat
    words, pool = 128 * 128 // 32, 4 * (128 * 128 // 32)
    # one capturing ship: the 17 rows of an arena then reach back 17 frames, further than its pool keeps them
    kw = dict(per=False, behaviours=["idle", "random", "random"] + ["idle"] * (M3 - 3), n_ships=M3, masked=(0,),
              dead=((3, 0),), **SMALL)
    d, p = _Twin(False, **kw), _Twin(True, pool, **kw)
    models = [PackedRing(FRAMES, pool) for _ in range(N)]
    dense_live = [dict() for _ in range(N)]                              # tick -> counts, the last FRAMES stored frames
    for t in range(T3):
        d.step(t, restart_every=15), p.step(t, restart_every=15)
        for a in range(N):
            try:
                s, l = d.b.replay_frame(a, t)
            except OfxError:
                continue
            k = (_nonzero_words(s), _nonzero_words(l))
            models[a].store(t, *k)
            dense_live[a][t] = k
            for old in sorted(dense_live[a])[:-FRAMES]:
                del dense_live[a][old]
    db, pb = d.b, p.b
    fd, fp = _frames(db, T3), _frames(pb, T3)
    # ---- the condition this test exists for: in at least two arenas some, and not all, of the dense twin's frames are gone
    gone = [len(set(fd[a]) - set(models[a].live_ticks())) for a in range(N)]
    print("dense frames", [len(f) for f in fd], "gone early", gone, "evicted", [m.evicted for m in models],
          "rows", [len(db.replay_rows(a)) for a in range(N)])
    assert sum(1 for a in range(N) if 0 < gone[a] < len(fd[a]) - 1) >= 2
    assert all(sorted(fd[a]) == sorted(dense_live[a]) for a in range(N))
    # ---- availability per tick, and the bytes of what is there
    for a in range(N):
        assert sorted(fp[a]) == models[a].live_ticks()
        assert all(fp[a][t] == fd[a][t] for t in fp[a])
    # ---- the store's numbers
    st = pb.replay_store_stats()
    assert (st["live_max"], st["live_sum"], st["evicted"]) == (max(m.live for m in models), sum(m.live for m in models),
                                                              sum(m.evicted for m in models))
    # ---- the samplers skip the rows whose state frame was evicted
    rows = [db.replay_rows(a) for a in range(N)]
    assert all(pb.replay_rows(a).tobytes() == rows[a].tobytes() for a in range(N))
    want_valid = [eligible(rows[a], models[a].frame_tick) for a in range(N)]
    assert any(0 < v < len(r) for v, r in zip(want_valid, rows))
    for batch in (4, 32):
        slot, n = pb.replay_sample(SEED, 1, batch)
        pb.sync()
        assert list(n.download(np.int32, (N,))) == [min(batch, v) for v in want_valid]
        g_rows, bp, bn = pb.replay_gather(slot, batch)
        for a in range(N):
            for j in range(batch):
                r = g_rows[a, j]
                if r["ship"] < 0:
                    assert not bp[a, j].any() and not bn[a, j].any()
                    continue
                for bits, tick in ((bp[a, j], int(r["tick_prev"])), (bn[a, j], int(r["tick_next"]))):
                    m = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(2, 128, 128)
                    assert (np.packbits(m[0]).tobytes(), np.packbits(m[1]).tobytes()) == fd[a][tick]
    # ---- the dense twin's memory does not fit this pool: refused, nothing touched
    before = pb.replay_export(0, 5).tobytes()
    with pytest.raises(OfxError, match=r"arena \d of the chunk hold \d+ pairs, the pool 2048") as err:
        pb.replay_import(0, 5, db.replay_export(0, 5))
    assert err.value.code == nat.OFX_ERR_INVALID
    assert pb.replay_export(0, 5).tobytes() == before and _frames(pb, T3) == fp
    # its own blob goes back in (re-packed from position 0) and into a dense handle
    pb.replay_import(0, 5, np.frombuffer(before, np.uint8))
    assert pb.replay_export(0, 5).tobytes() == before and _frames(pb, T3) == fp
    db.replay_import(0, 5, np.frombuffer(before, np.uint8))
    assert _frames(db, T3) == fp
    db.close(), pb.close()


# ------------------------------------------------------------------------------------------------------ 4. trainer
N4, M4, SEED4 = 4, 2, 0x0F160033
CONFIGS = {"defaults": {}, "everything": dict(prioritized=True, n_step=3, double_dqn=True, target_sync=2, huber_delta=1.0)}


def _build(cfg, packed):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N4, M4)
    eps = Epsilon_decay()
    eps.set(0.3)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=16,
                       packed_memory=packed, **CONFIGS[cfg])
    roll = TrainingRollout(b, tr, ["random"] * M4, SEED4, policy_ships=(0, 1), episode_ticks=20, collecting_steps=5,
                           replay_every=10)
    return b, tr, roll


def _trained(b, tr):
    b.sync()
    blob = lambda buf: buf.download(np.float32, (tr.n_floats,)).tobytes()
    return {"weights": blob(tr.weights), "adam_m": blob(tr.adam_m), "adam_v": blob(tr.adam_v),
            "target": None if tr.target is None else blob(tr.target), "losses": list(tr.losses),
            "fit_steps": tr.fit_steps, "draws": tr.draws, "count": b.replay_count()[0].tobytes(),
            "rows": [b.replay_rows(a).tobytes() for a in range(N4)]}


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_packed_trainer_fits_the_same_bits(tmp_path, cfg):
    bd, td, rd = _build(cfg, False)
    bp, tp, rp = _build(cfg, True)
    rd.run(30), rp.run(30)
    assert td.fit_steps >= 2 and all(np.isfinite(x).all() for x in td.losses)
    assert _differing(_trained(bd, td), _trained(bp, tp)) == []
    st = bp.replay_store_stats()
    assert st["packed"] == 1 and st["evicted"] == 0 and st["live_sum"] > 0 and bd.replay_store_stats()["packed"] == 0
    assert "packed_memory" not in tp.fingerprint() and tp.fingerprint() == td.fingerprint()
    # a checkpoint of the packed run, restored into a fresh packed run, continues bit for bit
    path = str(tmp_path / "ckpt")
    rp.checkpoint(path)
    bq, tq, rq = _build(cfg, True)
    rq.restore(path)
    assert _differing(_trained(bq, tq), _trained(bp, tp)) == []
    rp.run(10), rq.run(10), rd.run(10)
    end = _trained(bp, tp)
    assert tp.fit_steps > 3 and _differing(_trained(bq, tq), end) == [] and _differing(_trained(bd, td), end) == []
    assert bq.replay_export(0, N4).tobytes() == bp.replay_export(0, N4).tobytes() == bd.replay_export(0, N4).tobytes()
    bd.close(), bp.close(), bq.close()
