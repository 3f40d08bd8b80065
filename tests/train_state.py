"""A device-resident training run's whole state in comparable form - weights, moments, logs, counters, arenas, maps and
what the host inspections report of the replay memory - for the tests that compare two runs bit for bit.  A helper
module (not collected)."""
import numpy as np


def inspect_replay(b, ticks, arenas=None):
    """What the host inspections report: counts, appended, and per arena the rows, the masses and every held frame.
    arenas: inspect only these (the lists then hold None for the others)."""
    from ofighters_amd import OfxError
    cnt, app = b.replay_count()
    out = {"count": cnt, "appended": app, "rows": [], "mass": [], "frames": []}
    for a in range(b.N):
        if arenas is not None and a not in arenas:
            for k in ("rows", "mass", "frames"):
                out[k].append(None)
            continue
        out["rows"].append(b.replay_rows(a).tobytes())
        out["mass"].append(b.replay_priorities(a).tobytes() if b.replay_prioritized else None)
        held = {}
        for t in range(ticks):
            try:
                s, l = b.replay_frame(a, t)
                held[t] = (np.packbits(s).tobytes(), np.packbits(l).tobytes())
            except OfxError:
                pass
        out["frames"].append(held)
    return out


def _unpack(words, W, H):
    return np.packbits(np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little").reshape(H, W)).tobytes()


def check_decoded(d, ins, arena0, only=None):
    """The decoded chunk (tests/ckpt_blob.py) says what the inspections say about arenas [arena0, arena0 + n); only:
    compare these arenas of the handle alone (inspect_replay's `arenas`)."""
    W, H = d["W"], d["H"]
    for i in range(d["n"]):
        a = arena0 + i
        if only is not None and a not in only:
            continue
        cnt, head = int(d["count"][i]), int(d["head"][i])
        assert cnt == ins["count"][a] and d["appended"][i] == ins["appended"][a]
        order = (head - cnt + np.arange(cnt)) % d["C"]
        assert d["rows"][i][order].tobytes() == ins["rows"][a]
        assert d["mass"][i][order].tobytes() == ins["mass"][a]
        live = {int(t): s for s, t in enumerate(d["frame_tick"][i]) if t >= 0}
        assert sorted(live) == sorted(ins["frames"][a])
        for t, s in live.items():
            assert (_unpack(d["maps"][i, s, 0], W, H), _unpack(d["maps"][i, s, 1], W, H)) == ins["frames"][a][t], (a, t)
        for s, t in enumerate(d["frame_tick"][i]):
            if t < 0:
                assert d["counts"][i, s].sum() == 0


def training_state(b, tr, roll):
    """Everything the issue lists, in comparable form."""
    from ofighters_amd import _native as nat
    b.sync()
    s = {"weights": tr.weights_host().tobytes(), "adam_m": tr.adam_m.download(np.float32, (tr.n_floats,)).tobytes(),
         "adam_v": tr.adam_v.download(np.float32, (tr.n_floats,)).tobytes(),
         "target": None if tr.target is None else tr.target_host().tobytes(),
         "losses": list(tr.losses), "grad_norms": list(tr.grad_norms), "fit_steps": tr.fit_steps, "draws": tr.draws,
         "epsilon": tr.epsilon.get(), "score_log": [x.tolist() for x in roll.score_log], "epsilons": list(roll.epsilons),
         "roll_losses": list(roll.losses),
         "counters": (roll.tick, roll.total_steps, roll.capture_tick, roll.episode, b.episode, b.tick)}
    for f in range(19):
        s["field%d" % f] = b.get(f).tobytes()
    s["maps"] = [m.tobytes() for m in b.maps_host(nat.MAP_U8)]
    s["replay"] = inspect_replay(b, roll.capture_tick)
    s["replay"]["count"], s["replay"]["appended"] = s["replay"]["count"].tobytes(), s["replay"]["appended"].tobytes()
    return s
