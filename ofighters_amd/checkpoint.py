"""Checkpoints of a TrainingRollout: the one module that knows the file format.

A checkpoint is ONE file per handle / rank holding everything a training run needs to go on, in a fresh process, exactly
where it stopped - bit for bit (every random stream is a counter RNG keyed by seed, global arena and a tick / draw
counter, and a fit is reproducible to the bit, so nothing else is hidden):

    the manifest     format version; N, M, W, H, arena_base; the trainer's and the rollout's fingerprints (the arguments
                     that must match at restore); the rollout's counters; the index of the sections
    rollout/*        losses, epsilons, score_log, the `_seen_done` latch; rung_log only under an exploration ladder or
                     evaluation arenas (the ladder itself is re-derived by the constructor from the fingerprint's arguments);
                     span_reward (int32 [N][M], the last span's summed rewards) only under action_repeat > 1;
                     auto_sums (int64 [G][M+2], what the running reporting period has banked) and length_log only under
                     auto_reset
    autoreset/*      only under auto_reset: arena_episode (uint32 [N]) and dead_once (uint8 [N][M]) of
                     ofx_restart_finished
    arena/<field>    the 19 state fields of the arenas (ArenaBatch.state_dict)
    trainer/*        weights, Adam m and v, the target blob, the loss and gradient-norm lists (DeviceTrainer.state_dict)
    replay/<k>       the replay memory as ofx_replay_export blobs of consecutive arena chunks, each chosen from
                     ofx_replay_export_bytes to stay under CHUNK_BYTES of host memory
    replay_actor_values   only with the trainer's actor_priorities: (q_sa, p_sp) of every ship's previous_*, float32
                     [N][M][2] (the replay blob keeps its format and does not carry them)

Layout: the 8 bytes b"OFXCKPT1"; the sections' raw little-endian bytes, each starting at a multiple of 8; the manifest
as UTF-8 JSON; a 24-byte trailer = uint64 manifest offset, uint64 manifest length, b"OFXCKPT1" again.  The manifest comes
last so that the sections stream to disk one chunk at a time.  The same state gives the same bytes (no time stamps).

The file is written under a temporary name in the target's directory, flushed, fsync'ed and then os.replace'd over the
target: an interrupted write never damages the previous checkpoint.

Not carried (and not needed): the laser-overflow counter (it counts "since the last call"), the episode score sums
(every restart rewrites them before they are read), the observation maps (rasterised again from the state), the fit's
workspaces and every other scratch buffer.  A resume uses the same world size; resharding is out of scope.
"""
import json
import os
import struct

import numpy as np

MAGIC = b"OFXCKPT1"
FORMAT = 1
CHUNK_BYTES = 256 << 20          # cap of one replay chunk's blob on the host


class _Writer:
    def __init__(self, path):
        self.path = path
        self.tmp = "%s.tmp-%d" % (path, os.getpid())
        self.f = open(self.tmp, "wb")
        self.f.write(MAGIC)
        self.sections = {}

    def add(self, name, arr):
        a = np.ascontiguousarray(arr)
        if a.dtype.byteorder == ">":
            a = a.astype(a.dtype.newbyteorder("<"))
        pos = self.f.tell()
        if pos % 8:
            self.f.write(b"\0" * (8 - pos % 8))
            pos = self.f.tell()
        self.f.write(memoryview(a.reshape(-1).view(np.uint8)) if a.size else b"")
        self.sections[name] = {"dtype": a.dtype.str, "shape": list(a.shape), "offset": pos, "nbytes": int(a.nbytes)}

    def finish(self, manifest):
        manifest = dict(manifest, sections=self.sections)
        js = json.dumps(manifest, sort_keys=True).encode("utf-8")
        pos = self.f.tell()
        self.f.write(js)
        self.f.write(struct.pack("<QQ", pos, len(js)) + MAGIC)
        self.f.flush()
        os.fsync(self.f.fileno())
        self.f.close()
        os.replace(self.tmp, self.path)
        try:                                   # make the rename itself durable where the platform allows it
            fd = os.open(os.path.dirname(os.path.abspath(self.path)), os.O_RDONLY)
            try:
                os.fsync(fd)
            finally:
                os.close(fd)
        except OSError:
            pass

    def abort(self):
        try:
            self.f.close()
        finally:
            if os.path.exists(self.tmp):
                os.remove(self.tmp)


class Reader:
    """An open checkpoint: `.manifest` and `array(name)` (one section at a time, so a large memory never sits on the
    host as a whole)."""

    def __init__(self, path):
        self.path = path
        size = os.path.getsize(path)
        with open(path, "rb") as f:
            if size < 32 or f.read(8) != MAGIC:
                raise ValueError("%s is not a checkpoint (wrong magic)" % path)
            f.seek(size - 24)
            pos, n, tail = struct.unpack("<QQ8s", f.read(24))
            if tail != MAGIC or pos + n + 24 != size:
                raise ValueError("%s is not a complete checkpoint (bad trailer)" % path)
            f.seek(pos)
            self.manifest = json.loads(f.read(n).decode("utf-8"))
        if self.manifest.get("format") != FORMAT:
            raise ValueError("%s: checkpoint format %r, this version reads %d" % (path, self.manifest.get("format"), FORMAT))
        self.sections = self.manifest["sections"]

    def array(self, name):
        s = self.sections[name]
        dt = np.dtype(s["dtype"])
        count = int(np.prod(s["shape"], dtype=np.int64))
        if count == 0:
            return np.zeros(s["shape"], dt)
        return np.fromfile(self.path, dtype=dt, count=count, offset=s["offset"]).reshape(s["shape"])


def _plain(v):
    """JSON form of a fingerprint value (tuples and numpy scalars lose their type, nothing else)."""
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


def rollout_fingerprint(r):
    """The TrainingRollout arguments a restored run must have been built with."""
    fp = {"policy_ships": sorted(int(i) for i in np.flatnonzero(np.asarray(r.policy_mask)[0])),
          "behaviours": _plain(r.behaviours), "seed": int(r.seed), "episode_ticks": int(r.episode_ticks),
          "collecting_steps": _plain(r.collecting_steps), "replay_every": _plain(r.replay_every),
          "replay_on_death": bool(r.replay_on_death), "is_learning": bool(r.is_learning)}
    if getattr(r, "ladder_on", False):                   # only when on: a default rollout's key set stays as it was
        fp.update(epsilon_ladder=r.epsilon_ladder, eval_arenas=int(r.eval_arenas), total_arenas=int(r.total_arenas),
                  score_bands=int(r.score_bands))
    if getattr(r, "action_repeat", 1) > 1:
        fp["action_repeat"] = int(r.action_repeat)
    if getattr(r, "auto_reset", False):
        fp["auto_reset"] = True
    if getattr(r, "boltzmann", None) is not None:
        fp["boltzmann"] = [float(r.boltzmann[0]), float(r.boltzmann[1])]
    return fp


def dims(engine):
    return {"N": int(engine.N), "M": int(engine.M), "W": int(engine.W), "H": int(engine.H),
            "arena_base": int(engine.arena_base)}


def _replay_chunks(engine, cap):
    """(arena0, n, blob) over the whole memory, every blob under `cap` bytes (a single arena may exceed it)."""
    N = engine.N
    total = engine.replay_export_bytes(0, N)
    n = N if total <= cap else max(1, int(N * (0.75 * cap / total)))
    a = 0
    while a < N:
        k = min(n, N - a)
        while k > 1 and engine.replay_export_bytes(a, k) > cap:
            k = max(1, k // 2)
        yield a, k, engine.replay_export(a, k)
        a += k


def save(rollout, path, chunk_bytes=None):
    """Write the rollout's checkpoint to `path` (replacing a previous one only once the new one is complete)."""
    e, t = rollout.e, rollout.trainer
    e.sync()
    w = _Writer(path)
    try:
        ts = t.state_dict()
        es = e.state_dict()
        manifest = {"format": FORMAT, "dims": dims(e), "trainer_fingerprint": _plain(ts["fingerprint"]),
                    "rollout_fingerprint": rollout_fingerprint(rollout),
                    "counters": {"tick": int(rollout.tick), "total_steps": int(rollout.total_steps),
                                 "capture_tick": int(rollout.capture_tick), "episode": int(rollout.episode),
                                 "engine_episode": int(es["episode"]), "engine_tick": int(es["tick"])},
                    "trainer": {"fit_steps": int(ts["fit_steps"]), "draws": int(ts["draws"]), "epsilon": _plain(ts["epsilon"]),
                                "has_target": ts["target"] is not None}}
        w.add("rollout/losses", np.array(rollout.losses, np.float64))
        w.add("rollout/epsilons", np.array(rollout.epsilons, np.float64))
        w.add("rollout/score_log", np.array(rollout.score_log, np.int64).reshape(len(rollout.score_log), e.M + 1))
        w.add("rollout/seen_done", rollout._seen_done.download(np.uint8, (e.N, e.M)))
        if getattr(rollout, "ladder_on", False):
            w.add("rollout/rung_log", np.array(rollout.rung_log, np.int64).reshape(len(rollout.rung_log), rollout.n_groups,
                                                                                   e.M + 1))
        if getattr(rollout, "action_repeat", 1) > 1:
            w.add("rollout/span_reward", rollout._span.download(np.int32, (e.N, e.M)))
        if getattr(rollout, "auto_reset", False):
            ar = e.autoreset_state()
            w.add("autoreset/arena_episode", ar["arena_episode"])
            w.add("autoreset/dead_once", ar["dead_once"])
            w.add("rollout/auto_sums", rollout._auto_sums.download(np.int64, (rollout._auto_groups, e.M + 2)))
            w.add("rollout/length_log", np.array(rollout.length_log, np.int64).reshape(len(rollout.length_log),
                                                                                       rollout._auto_groups))
        for name, a in es.items():
            if name not in ("episode", "tick"):
                w.add("arena/" + name, a)
        for name in ("weights", "adam_m", "adam_v", "target", "losses", "grad_norms"):
            if ts[name] is not None:
                w.add("trainer/" + name, ts[name])
        chunks = []
        for a, k, blob in _replay_chunks(e, chunk_bytes or CHUNK_BYTES):
            w.add("replay/%d" % len(chunks), blob)
            chunks.append([int(a), int(k)])
        manifest["replay_chunks"] = chunks
        if getattr(t, "actor_priorities", False):
            w.add("replay_actor_values", e.replay_actor_values())
        w.finish(manifest)
    except BaseException:
        w.abort()
        raise
    return path


def check(rollout, manifest):
    """ValueError listing every key on which the checkpoint and the rollout it is restored into disagree."""
    from .trainer import fingerprint_diff
    bad = []
    for group, have, want in (("dims", dims(rollout.e), manifest["dims"]),
                              ("trainer", _plain(rollout.trainer.fingerprint()), manifest["trainer_fingerprint"]),
                              ("rollout", rollout_fingerprint(rollout), manifest["rollout_fingerprint"])):
        bad += ["%s.%s (%r here, %r in the checkpoint)" % (group, k, have.get(k), want.get(k))
                for k in fingerprint_diff(have, want)]
    if bad:
        raise ValueError("the checkpoint was written by a differently built run: " + "; ".join(bad))


def load(rollout, path):
    """Restore `path` into a freshly constructed rollout built with the same arguments.  Fingerprints and dimensions
    are compared before anything is touched."""
    rd = Reader(path)
    m = rd.manifest
    check(rollout, m)
    e, t = rollout.e, rollout.trainer
    e.sync()
    for i, (a, k) in enumerate(m["replay_chunks"]):
        e.replay_import(a, k, rd.array("replay/%d" % i))
    if getattr(t, "actor_priorities", False):                          # (the fingerprints agree: the section is there)
        e.set_replay_actor_values(rd.array("replay_actor_values"))
    es = {name[len("arena/"):]: rd.array(name) for name in rd.sections if name.startswith("arena/")}
    es["episode"], es["tick"] = m["counters"]["engine_episode"], m["counters"]["engine_tick"]
    e.load_state_dict(es)
    ts = dict(m["trainer"], fingerprint=m["trainer_fingerprint"])
    for name in ("weights", "adam_m", "adam_v", "losses", "grad_norms"):
        ts[name] = rd.array("trainer/" + name)
    ts["target"] = rd.array("trainer/target") if m["trainer"]["has_target"] else None
    t.load_state_dict(ts)
    c = m["counters"]
    rollout.tick, rollout.total_steps, rollout.capture_tick = c["tick"], c["total_steps"], c["capture_tick"]
    rollout.episode = c["episode"]
    rollout.losses = [float(x) for x in rd.array("rollout/losses")]
    rollout.epsilons = [float(x) for x in rd.array("rollout/epsilons")]
    rollout.score_log = [row.copy() for row in rd.array("rollout/score_log")]
    if getattr(rollout, "ladder_on", False):                           # (the fingerprints agree: the section is there)
        rollout.rung_log = [g.copy() for g in rd.array("rollout/rung_log")]
    e.sync()
    rollout._seen_done.upload(rd.array("rollout/seen_done"))
    if getattr(rollout, "action_repeat", 1) > 1:                       # (the fingerprints agree: the section is there)
        rollout._span.upload(rd.array("rollout/span_reward"))          # the next capture's completed rows read it
    if getattr(rollout, "auto_reset", False):                          # (the fingerprints agree: the sections are there)
        e.load_autoreset_state({"arena_episode": rd.array("autoreset/arena_episode"),
                                "dead_once": rd.array("autoreset/dead_once")})
        e.sync()
        rollout._auto_sums.upload(rd.array("rollout/auto_sums"))       # the running reporting period goes on
        rollout.length_log = [g.copy() for g in rd.array("rollout/length_log")]
    e.policy_pin_weights(t.weights.ptr)             # the blob changed under the pin: prepare it again
    return m
