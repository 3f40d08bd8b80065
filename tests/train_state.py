"""A device-resident training run's whole state in comparable form - weights, moments, logs, counters, arenas, maps and
what the host inspections report of the replay memory - for the tests that compare two runs bit for bit.  A helper
module (not collected)."""
import numpy as np


def inspect_replay(b, ticks):
    """What the host inspections report: counts, appended, and per arena the rows, the masses and every held frame."""
    from ofighters_amd import OfxError
    cnt, app = b.replay_count()
    out = {"count": cnt, "appended": app, "rows": [], "mass": [], "frames": []}
    for a in range(b.N):
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
