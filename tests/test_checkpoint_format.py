"""Checkpoints without a device: ofx_replay_blob_check (host only) against blobs built by tests/ckpt_blob.py from the
layout text of include/ofx.h, the epsilon schedules' state, and TrainingRollout.checkpoint / restore on the stand-ins
of tests/checkpoint_standin.py (those of tests/rollout_standin.py extended by what a checkpoint needs)."""
import ctypes as C
import json

import numpy as np
import pytest

from ofighters_amd import _native as nat
from tests import ckpt_blob
from tests.checkpoint_standin import (ROLLOUT_KEYS, TRAINER_KEYS, HostBuffer as _HostBuffer, host_trainer as _trainer,
                                       standins as _standins)

W = H = 400
WORDS = W * H // 32
DIMS = dict(n_ships=3, width=W, height=H, capacity=4, frames=6, prioritized=1, n_arenas=2)


def blob_check(blob, **kw):
    a = dict(DIMS, **kw)
    b = np.frombuffer(bytes(blob), np.uint8)
    rc = nat.lib().ofx_replay_blob_check(b.ctypes.data_as(C.c_void_p), b.nbytes, a["n_ships"], a["width"], a["height"],
                                         a["capacity"], a["frames"], a["prioritized"], a["n_arenas"])
    return rc, nat.lib().ofx_last_error().decode()


def example():
    """2 arenas, M = 3, capacity 4, frames 6 at 400 x 400 with PER: empty slots, an all-zero stored map, a map with its
    first and last word set, one with > 64 and one with > 256 nonzero words."""
    n, M, Cc, F = 2, 3, 4, 6
    rng = np.random.default_rng(5)
    d = dict(W=W, H=H, M=M, C=Cc, F=F, n=n, per=1, alpha=np.float32(0.6), eps=np.float32(1e-3))
    d["frame_tick"] = np.array([[0, 1, 2, 3, -1, -1], [6, 7, 2, 3, 4, 5]], np.int32)
    d["frame_head"] = np.array([4, 2], np.int32)
    d["cur_slot"] = np.array([3, -1], np.int32)
    maps = np.zeros((n, F, 2, WORDS), np.uint32)
    maps[0, 0, 0, 0], maps[0, 0, 0, WORDS - 1] = 1, 0x80000000          # first and last word (slot 0 1: all-zero map)
    maps[0, 2, 1, rng.choice(WORDS, 100, replace=False)] = rng.integers(1, 2**32, 100, dtype=np.uint64).astype(np.uint32)
    maps[0, 3, 0, rng.choice(WORDS, 300, replace=False)] = rng.integers(1, 2**32, 300, dtype=np.uint64).astype(np.uint32)
    for f in range(F):
        maps[1, f, :, rng.choice(WORDS, 7, replace=False)] = 0xFF
    d["maps"] = maps
    rows = np.zeros((n, Cc), ckpt_blob.TRANSITION)
    for a in range(n):
        for i in range(Cc):
            rows[a, i] = (i, i + 1, i % F, (i + 1) % F, i % M, i % 2, 17 * i, H - 1 - i, 1, 0, np.arange(8), np.arange(8) + 1)
    rows[0, 3]["frame_next"], rows[0, 3]["ship"], rows[0, 3]["px"] = 99, -5, 4000   # stale (count 3, head 3): not checked
    d["rows"] = rows
    d["head"], d["count"] = np.array([3, 2], np.int32), np.array([3, 4], np.int32)
    d["appended"] = np.array([3, 10], np.int64)
    d["has_prev"] = np.array([[1, 0, 1], [0, 0, 1]], np.uint8)
    d["latched"] = np.array([[0, 0, 1], [0, 1, 0]], np.uint8)
    d["prev_iaction"] = np.array([[1, 7, 0], [9, 9, 1]], np.int32)          # 7 / 9: ships without previous_*
    d["prev_px"] = np.full((n, M), W - 1, np.int32)
    d["prev_py"] = np.zeros((n, M), np.int32)
    d["prev_tick"] = np.full((n, M), 3, np.int32)
    d["prev_slot"] = np.array([[3, -1, 3], [77, 0, 5]], np.int32)
    d["prev_head"] = rng.random((n, M, 8)).astype(np.float32)
    d["mass"] = rng.random((n, Cc)).astype(np.float32)
    d["mmax"] = np.array([1.0, 2.5], np.float32)
    return d


@pytest.fixture(scope="module")
def good():
    d = example()
    blob = ckpt_blob.encode(d)
    return d, blob, ckpt_blob.layout(d)


def test_blob_check_accepts_an_encoded_blob_and_decode_round_trips(good):
    d, blob, lay = good
    rc, msg = blob_check(blob)
    assert rc == nat.OFX_OK, msg
    back = ckpt_blob.decode(blob)
    for k, v in d.items():
        assert np.array_equal(back[k], v), k
    cnt = back["counts"]
    assert cnt[0, 0, 0] == 2 and cnt[0, 1].sum() == 0 and cnt[0, 4:].sum() == 0 and cnt[0, 2, 1] == 100 and cnt[0, 3, 0] == 300
    d0 = dict(d, per=0)                                  # the same memory without PER: no mass / mmax arrays
    rc, msg = blob_check(ckpt_blob.encode(d0), prioritized=0)
    assert rc == nat.OFX_OK, msg


def _poke(blob, at, fmt, *v):
    import struct
    b = bytearray(blob)
    struct.pack_into(fmt, b, at, *v)
    return bytes(b)


def _row_field(lay, arena, pos, field, Cc=4):
    return lay["rows"][0] + (arena * Cc + pos) * 104 + ckpt_blob.TRANSITION.fields[field][1]


def _faults(d, blob, lay):
    """(label, corrupt blob, dims override, word the message must hold)"""
    pairs, counts = lay["pairs"], lay["counts"]
    out = [("magic", _poke(blob, 0, "<I", 0x12345678), {}, "magic"),
           ("version", _poke(blob, 4, "<I", 2), {}, "version"),
           ("words in the header", _poke(blob, 28, "<i", WORDS + 4), {}, "words"),
           ("short header", blob[:79], {}, "truncated"),
           ("raw boundary", blob[:80], {}, "truncated"),
           ("count boundary", blob[:counts], {}, "truncated"),
           ("pair boundary", blob[:pairs], {}, "truncated"),
           ("one byte short", blob[:-1], {}, "truncated"),
           ("one byte long", blob + b"\0", {}, "sections end"),
           ("count > words", _poke(blob, counts, "<I", WORDS + 1), {}, "exceeds"),
           ("count in an empty slot", _poke(blob, counts + 4 * (4 * 2), "<I", 1), {}, "empty slot"),
           ("counts do not sum", _poke(blob, counts + 4 * 2, "<I", 1), {}, "sum to"),
           ("index == words", _poke(blob, pairs + 8, "<I", WORDS), {}, "word index"),
           ("equal indices", _poke(blob, pairs + 8, "<I", 0), {}, "ascend"),
           ("descending indices", _poke(blob, pairs + 16 + 8, "<I", 0), {}, "ascend"),
           ("zero word", _poke(blob, pairs + 4, "<I", 0), {}, "zero word"),
           ("head == capacity", _poke(blob, lay["head"][0], "<i", 4), {}, "head"),
           ("frame_head == frames", _poke(blob, lay["frame_head"][0] + 4, "<i", 6), {}, "frame_head"),
           ("cur_slot == frames", _poke(blob, lay["cur_slot"][0], "<i", 6), {}, "cur_slot"),
           ("count > capacity", _poke(blob, lay["count"][0] + 4, "<i", 5), {}, "count"),
           ("appended < count", _poke(blob, lay["appended"][0], "<q", 2), {}, "appended"),
           ("frame_tick == -2", _poke(blob, lay["frame_tick"][0] + 4 * 5, "<i", -2), {}, "frame_tick"),
           ("live frame_next == frames", _poke(blob, _row_field(lay, 0, 1, "frame_next"), "<i", 6), {}, "frame_next"),
           ("live frame_prev == -1", _poke(blob, _row_field(lay, 1, 3, "frame_prev"), "<i", -1), {}, "frame_prev"),
           ("live ship == M", _poke(blob, _row_field(lay, 0, 2, "ship"), "<i", 3), {}, "ship"),
           ("live px == W", _poke(blob, _row_field(lay, 1, 0, "px"), "<i", W), {}, "px"),
           ("live py == H", _poke(blob, _row_field(lay, 0, 0, "py"), "<i", H), {}, "py"),
           ("live iaction == 2", _poke(blob, _row_field(lay, 0, 0, "iaction"), "<i", 2), {}, "iaction"),
           ("prev_slot of a ship with previous_*", _poke(blob, lay["prev_slot"][0], "<i", 6), {}, "prev_slot"),
           ("NaN mass", _poke(blob, lay["mass"][0] + 4 * 5, "<f", float("nan")), {}, "mass"),
           ("negative mmax", _poke(blob, lay["mmax"][0], "<f", -1.0), {}, "mmax")]
    for key, val, word in (("n_ships", 4, "n_ships"), ("width", 800, "width"), ("height", 800, "height"),
                           ("capacity", 5, "capacity"), ("frames", 7, "frames"), ("prioritized", 0, "prioritized"),
                           ("n_arenas", 3, "n_arenas")):
        kw = {key: val}
        if key == "width":
            kw["height"] = 200                           # the same number of words: the width itself is what differs
        out.append(("argument %s" % key, blob, kw, word))
    return out


def test_blob_check_refuses_every_fault_and_recovers(good):
    d, blob, lay = good
    assert ckpt_blob.decode(blob)["counts"][0, 0, 0] == 2          # the first three pairs: map (0, 0, 0) then (0, 2, 1)
    faults = _faults(d, blob, lay)
    assert len(faults) >= 35
    for label, bad, kw, word in faults:
        rc, msg = blob_check(bad, **kw)
        assert rc == nat.OFX_ERR_INVALID, label
        assert msg.startswith("ofx_replay_blob_check") and word in msg, (label, msg)
        rc, msg = blob_check(blob)                                  # no refusal leaves a later accepting call affected
        assert rc == nat.OFX_OK, (label, msg)


def test_blob_check_reads_an_unaligned_blob(good):
    _, blob, _ = good
    buf = np.zeros(len(blob) + 9, np.uint8)
    buf[3:3 + len(blob)] = np.frombuffer(blob, np.uint8)
    a = DIMS
    rc = nat.lib().ofx_replay_blob_check(C.c_void_p(buf.ctypes.data + 3), len(blob), a["n_ships"], a["width"], a["height"],
                                         a["capacity"], a["frames"], a["prioritized"], a["n_arenas"])
    assert rc == nat.OFX_OK, nat.lib().ofx_last_error()


# -------------------------------------------------------------------------------- stitching the dicts of chunks
def _synthetic(n, w, h, per, seed, M=3, Cc=5, F=7):
    """A memory of n arenas on w x h maps that no device wrote: empty slots, all-zero stored maps, full maps, the first
    and the last word set, arenas without rows."""
    rng = np.random.default_rng(seed)
    words = w * h // 32
    d = dict(W=w, H=h, M=M, C=Cc, F=F, n=n, per=per, alpha=np.float32(0.7), eps=np.float32(1e-2))
    d["frame_tick"] = rng.integers(-1, 50, (n, F)).astype(np.int32)
    d["frame_tick"][n // 2] = -1                                       # an arena whose ring is empty
    d["frame_tick"][0, 0], d["frame_tick"][n - 1, F - 1] = 3, 4
    maps = rng.integers(0, 2**32, (n, F, 2, words), dtype=np.uint64).astype(np.uint32)
    maps[rng.random((n, F, 2, words)) < 0.6] = 0
    maps[rng.random((n, F, 2)) < 0.2] = 0                              # all-zero stored maps
    maps[0, 0, 0], maps[n - 1, F - 1, 1] = 0xFFFFFFFF, 0x80000001      # every word set; the last map of the chunk
    maps[d["frame_tick"] < 0] = 0
    d["maps"] = maps
    rows = np.zeros((n, Cc), ckpt_blob.TRANSITION)
    rows.view(np.uint8)[:] = rng.integers(0, 256, rows.view(np.uint8).shape, dtype=np.uint8)
    d["rows"] = rows
    for k in ("frame_head", "cur_slot", "head", "count"):
        d[k] = rng.integers(0, Cc, n).astype(np.int32)
    d["appended"] = rng.integers(0, 2**40, n).astype(np.int64)
    d["has_prev"], d["latched"] = (rng.integers(0, 2, (n, M)).astype(np.uint8) for _ in range(2))
    for k in ("prev_iaction", "prev_px", "prev_py", "prev_tick", "prev_slot"):
        d[k] = rng.integers(0, 1000, (n, M)).astype(np.int32)
    d["prev_head"] = rng.random((n, M, 8)).astype(np.float32)
    if per:
        d["mass"], d["mmax"] = rng.random((n, Cc)).astype(np.float32), rng.random(n).astype(np.float32)
    return d


def _chunk(d, lo, hi):
    out = {k: v for k, v in d.items() if not isinstance(v, np.ndarray) or v.ndim == 0}
    out.update({k: v[lo:hi] for k, v in d.items() if isinstance(v, np.ndarray) and v.ndim})
    out["n"] = hi - lo
    return out


@pytest.mark.parametrize("per", [0, 1])
@pytest.mark.parametrize("w,h", [(16, 8), (32, 32)])
def test_concat_of_decoded_chunks_is_the_spanning_chunk(w, h, per):
    """7 arenas cut into 2 + 5 and into 4 + 1 + 2: the chunks' blobs decoded, stitched and encoded are the blob of the
    whole, byte for byte - odd array sizes, so the 8-byte padding of the raw arrays differs between chunk and whole."""
    ab = _synthetic(7, w, h, per, seed=w + per)
    whole = ckpt_blob.encode(ab)
    for cuts in ((0, 2, 7), (0, 4, 5, 7)):
        parts = [_chunk(ab, lo, hi) for lo, hi in zip(cuts, cuts[1:])]
        blobs = [ckpt_blob.encode(p) for p in parts]
        assert len(set(len(b) for b in blobs)) == len(blobs)           # unequal parts
        got = ckpt_blob.concat([ckpt_blob.decode(ckpt_blob.encode(p)) for p in parts])
        assert got["n"] == 7 and np.array_equal(got["counts"], ckpt_blob.decode(whole)["counts"])
        assert ckpt_blob.encode(got) == whole
    assert ckpt_blob.encode(ckpt_blob.concat([ckpt_blob.decode(whole)])) == whole
    other = _chunk(_synthetic(7, w, h, per, seed=1, Cc=6), 0, 2)       # a chunk of another memory: refused
    with pytest.raises(AssertionError):
        ckpt_blob.concat([ckpt_blob.decode(ckpt_blob.encode(parts[0])), ckpt_blob.decode(ckpt_blob.encode(other))])


# ---------------------------------------------------------------------------------------------- epsilon schedules
@pytest.mark.parametrize("make", ["cos", "decay", "cos_set"])
def test_epsilon_state_round_trips(make):
    from ofighters_amd.lib.epsilon import Epsilon_cos, Epsilon_decay
    from ofighters_amd.trainer import epsilon_state, set_epsilon_state
    new = (lambda: Epsilon_cos(7)) if make != "decay" else Epsilon_decay
    e = new()
    if make == "cos_set":
        e.set(0.3)                                       # t becomes a float
    for _ in range(10):
        e.next()
    state = json.loads(json.dumps(epsilon_state(e)))     # through the manifest's JSON
    assert state["class"] == type(e).__name__
    f = new()
    set_epsilon_state(f, state)
    assert f.get() == e.get() and vars(f) == vars(e)
    assert [f.next() for _ in range(20)] == [e.next() for _ in range(20)]
    with pytest.raises(ValueError):
        set_epsilon_state(Epsilon_decay() if make != "decay" else Epsilon_cos(7), state)


# ------------------------------------------------------------------- TrainingRollout.checkpoint / restore, stand-ins
def test_checkpoint_manifest_round_trips(tmp_path, monkeypatch):
    from ofighters_amd import checkpoint
    r, e, t, _ = _standins(monkeypatch, tmp_path)
    r.run(93)                                            # two episode ends, mid-episode, one death latched this episode
    path = str(tmp_path / "ck")
    monkeypatch.setattr(checkpoint, "CHUNK_BYTES", 11)   # two arenas per chunk: [0, 2) and [2, 3)
    r.checkpoint(path)
    rd = checkpoint.Reader(path)
    m = rd.manifest
    assert m["format"] == 1 and m["dims"] == {"N": 3, "M": 2, "W": 400, "H": 400, "arena_base": 0}
    assert tuple(sorted(m["trainer_fingerprint"])) == tuple(sorted(TRAINER_KEYS)) and m["trainer_fingerprint"] == t.fingerprint()
    assert tuple(sorted(m["rollout_fingerprint"])) == tuple(sorted(ROLLOUT_KEYS))
    assert m["rollout_fingerprint"]["policy_ships"] == [0] and m["rollout_fingerprint"]["behaviours"] == ["idle", "idle"]
    assert m["counters"] == {"tick": 93, "total_steps": 93, "capture_tick": 93, "episode": 2, "engine_episode": 2,
                             "engine_tick": 13}
    assert m["replay_chunks"] == [[0, 2], [2, 1]]
    assert np.array_equal(rd.array("rollout/score_log"), np.array(r.score_log)) and rd.array("rollout/score_log").shape == (2, 3)
    assert np.array_equal(rd.array("rollout/seen_done"), r._seen_done.data) and rd.array("rollout/seen_done").shape == (3, 2)
    assert rd.array("rollout/losses").tolist() == r.losses and rd.array("rollout/epsilons").tolist() == r.epsilons
    # into a freshly built rollout: everything comes back, and both continue alike
    r2, e2, t2, up2 = _standins(monkeypatch, tmp_path)
    assert r2.restore(path) == m
    assert up2 == ["replay:0:2", "replay:2:1", "arena", "trainer", "buffer"] and e2.log[-1] == "pin"
    assert (r2.tick, r2.total_steps, r2.capture_tick, r2.episode) == (93, 93, 93, 2)
    assert r2.losses == r.losses and r2.epsilons == r.epsilons and np.array_equal(r2.score_log, r.score_log)
    assert np.array_equal(e2.memory, e.memory) and np.array_equal(t2.w, t.w) and t2.epsilon.n == t.epsilon.n
    e2.seen, r2._seen_done.cleared = e.seen.copy(), False    # (the stand-in keeps its latches on the host)
    n0 = len(e.log)
    r.run(40), r2.run(40)
    assert e2.log[-(len(e.log) - n0):] == e.log[n0:] and len(t2.replays) == len(t.replays)
    assert r2.losses == r.losses and r2.episode == r.episode == 3
    # the same state gives the same bytes
    r.checkpoint(str(tmp_path / "a")), r.checkpoint(str(tmp_path / "b"))
    assert open(str(tmp_path / "a"), "rb").read() == open(str(tmp_path / "b"), "rb").read()


def _changed(group, key):
    """Constructor changes of the stand-ins that alter exactly one fingerprint key."""
    if group == "trainer":
        return dict(trainer_fp={key: 0.25 if key == "target_tau" else 7})
    if group == "dims":
        return dict(engine_kw={"arena_base": 96}) if key == "arena_base" else None
    return {"policy_ships": dict(policy_ships=(1,)), "behaviours": dict(behaviours=["idle", "random"]), "seed": dict(seed=4),
            "episode_ticks": dict(episode_ticks=41), "collecting_steps": dict(collecting_steps=21),
            "replay_every": dict(replay_every=51), "replay_on_death": dict(replay_on_death=False),
            "is_learning": dict(is_learning=False)}[key]


@pytest.mark.parametrize("group,key", [("trainer", k) for k in TRAINER_KEYS] + [("rollout", k) for k in ROLLOUT_KEYS]
                         + [("dims", "arena_base"), ("dims", "N"), ("dims", "M"), ("dims", "W")])
def test_restore_refuses_every_fingerprint_key_before_any_upload(tmp_path, monkeypatch, group, key):
    r, e, t, _ = _standins(monkeypatch, tmp_path)
    r.run(30)
    path = str(tmp_path / "ck")
    r.checkpoint(path)
    kw = _changed(group, key)
    if kw is None:
        kw = dict(engine_kw={"N": 4} if key == "N" else {"M": 3} if key == "M" else {})
        if key == "M":
            kw["behaviours"] = ["idle"] * 3
    r2, e2, t2, up2 = _standins(monkeypatch, tmp_path, **kw)
    if key == "W":
        e2.W = 800
    before = (e2.memory.copy(), t2.w.copy(), r2.tick)
    with pytest.raises(ValueError) as err:
        r2.restore(path)
    assert "%s.%s " % (group, key) in str(err.value), str(err.value)
    assert str(err.value).count(" here, ") == 1 + (key == "M" and group == "dims")   # (M also changes the behaviours list)
    assert up2 == [] and r2.tick == before[2] and np.array_equal(e2.memory, before[0]) and np.array_equal(t2.w, before[1])


def test_interrupted_write_leaves_the_previous_checkpoint(tmp_path, monkeypatch):
    import os
    from ofighters_amd import checkpoint
    r, e, t, _ = _standins(monkeypatch, tmp_path)
    monkeypatch.setattr(checkpoint, "CHUNK_BYTES", 4)    # one arena per chunk
    r.run(30)
    folder = tmp_path / "ck"
    folder.mkdir()
    path = str(folder / "checkpoint-latest")
    r.checkpoint(path)
    first = open(path, "rb").read()
    r.run(30)
    e.fail_export = True                                 # the second chunk's export raises in the middle of the write
    with pytest.raises(RuntimeError, match="export interrupted"):
        r.checkpoint(path)
    assert open(path, "rb").read() == first and os.listdir(str(folder)) == ["checkpoint-latest"]
    r2, e2, t2, _ = _standins(monkeypatch, tmp_path)
    assert r2.restore(path)["counters"]["tick"] == 30
    e.fail_export = False
    r.checkpoint(path)
    assert checkpoint.Reader(path).manifest["counters"]["tick"] == 60
    # a truncated file is refused as a whole
    open(str(folder / "cut"), "wb").write(first[:-5])
    with pytest.raises(ValueError):
        checkpoint.Reader(str(folder / "cut"))


def test_checkpoint_every_writes_at_episode_ends(tmp_path, monkeypatch):
    import os
    folder = str(tmp_path / "auto")
    r, e, t, _ = _standins(monkeypatch, tmp_path, checkpoint_every=2, checkpoint_folder=folder)
    r.run(79)
    assert not os.path.exists(folder)                    # episode 1 is not a second one, episode 2 not complete
    r.run(1)
    assert os.listdir(folder) == ["checkpoint-latest"]
    auto = open(os.path.join(folder, "checkpoint-latest"), "rb").read()
    r.checkpoint(str(tmp_path / "manual"))
    assert open(str(tmp_path / "manual"), "rb").read() == auto
    r.run(39)                                            # episode 3 completes without a checkpoint
    assert open(os.path.join(folder, "checkpoint-latest"), "rb").read() == auto


# ------------------------------------------------------------------------- DeviceTrainer's own fingerprint and state
def test_device_trainer_state_round_trips_on_host_buffers(monkeypatch):
    a = _trainer(monkeypatch)
    assert tuple(sorted(a.fingerprint())) == tuple(sorted(TRAINER_KEYS))
    a.adam_m.upload(np.full(6, 2, np.float32)), a.adam_v.upload(np.full(6, 3, np.float32))
    a.target.upload(np.full(6, 4, np.float32))
    a.fit_steps, a.draws, a.losses, a.grad_norms = 5, 7, [(0.5, 0.25)] * 5, [1.5] * 5
    for _ in range(9):
        a.decay_epsilon()
    d = a.state_dict()
    b = _trainer(monkeypatch)
    ptrs = (b.weights, b.adam_m, b.adam_v, b.target)
    b.load_state_dict(d)
    assert (b.weights, b.adam_m, b.adam_v, b.target) == ptrs            # uploaded into the existing buffers
    d2 = b.state_dict()
    for k in ("weights", "adam_m", "adam_v", "target", "losses", "grad_norms"):
        assert np.array_equal(d[k], d2[k]) and d[k].dtype == d2[k].dtype, k
    assert (b.fit_steps, b.draws, b.losses, b.grad_norms) == (5, 7, [(0.5, 0.25)] * 5, [1.5] * 5)
    assert b.epsilon.get() == a.epsilon.get() and d2["epsilon"] == d["epsilon"] and d2["fingerprint"] == d["fingerprint"]


@pytest.mark.parametrize("key,kw", [
    ("n_floats", dict(n_floats=7)), ("learning_rate", dict(learning_rate=2e-3)), ("gamma", dict(gamma=0.8)),
    ("batch_size", dict(batch_size=5)), ("fit_batch", dict(fit_batch=17)), ("seed", dict(seed=6)),
    ("reference_quirks", dict(reference_quirks=True, prioritized=False, n_step=1, target_sync=0, double_dqn=False,
                              huber_delta=None, clip_norm=None)),
    ("prioritized", dict(prioritized=False)), ("per_alpha", dict(per_alpha=0.7)), ("per_beta", dict(per_beta=0.5)),
    ("per_beta_steps", dict(per_beta_steps=10)), ("per_eps", dict(per_eps=1e-2)), ("n_step", dict(n_step=2)),
    ("target_sync", dict(target_sync=3)), ("target_tau", dict(target_sync=0, target_tau=0.5)),
    ("double_dqn", dict(double_dqn=False)), ("huber_delta", dict(huber_delta=2.0)), ("clip_norm", dict(clip_norm=None)),
    ("memory_capacity", dict(memory_size=17, frames=22)), ("memory_frames", dict(frames=30))])
def test_device_trainer_refuses_other_hyperparameters_before_any_write(monkeypatch, key, kw):
    gamma = kw.pop("gamma", None)
    d = _trainer(monkeypatch).state_dict()
    b = _trainer(monkeypatch, **kw)
    if gamma is not None:
        b.gamma = gamma
    del _HostBuffer.log[:]
    before = b.state_dict()
    with pytest.raises(ValueError) as err:
        b.load_state_dict(d)
    assert key + " (" in str(err.value), str(err.value)
    if key not in ("reference_quirks", "target_tau"):               # (these two cannot change alone)
        assert str(err.value).count(" here, ") == 1, str(err.value)
    after = b.state_dict()
    assert _HostBuffer.log == [] and all(np.array_equal(before[k], after[k]) for k in ("weights", "adam_m", "adam_v"))
    assert (b.fit_steps, b.draws) == (0, 0)
