"""Soft and Munchausen targets on the device (include/ofx.h, "soft and Munchausen targets"): ofx_policy_forward_obs_soft
against the float64 log-sum-exp of the heat map the same call wrote, against ofx_policy_forward_obs where the two must
agree bit for bit, on every pixel once (T = 1e30), on the frame and row by row; ofx_dqn_targets_soft against the float64
formulas of tests/soft_oracle.py and against ofx_dqn_targets / _nstep; DeviceTrainer's two options through a rollout with
a checkpoint in the middle.

The observations are the 9 hand-built ones of tests/soft_oracle.py (one full group of 8 ships for the head kernel and
one group with a single live ship; every ship is 2 workgroups x 4 waves, so the 8-slot merge always runs), the weights
synthetic(7)."""
import numpy as np
import pytest

from tests import soft_oracle as so
from tests.frame_cases import CASES, frame_weights, where

pytestmark = pytest.mark.gpu

W = H = 400
NOBS = so.N_OBS
TAUS = (0.001, 0.03, 0.3, 1.0, 30.0)
SHARED = ("act", "iaction", "ipointer", "ptr_max", "ptr_probe")
PROBES = np.array([[0, 0], [399, 399], [199, 200], [200, 199], [37, 0], [0, 262], [399, 91], [137, 399], [250, 123]], np.int32)
_STATE = {}


def _rig():
    """One handle, the weights, the 9 observations and their probes on the device.  Kept for the module."""
    if "rig" not in _STATE:
        from ofighters_amd import ArenaBatch, DeviceBuffer
        from ofighters_amd.agents.policy_weights import synthetic
        b = ArenaBatch(2, 2)
        bits, vec8 = so.observations()
        w = synthetic(7)
        _STATE["rig"] = dict(b=b, w=DeviceBuffer(w.nbytes).upload(w), bits=DeviceBuffer(bits.nbytes).upload(bits),
                             vec8=DeviceBuffer(vec8.nbytes).upload(vec8), probe=DeviceBuffer(PROBES.nbytes).upload(PROBES),
                             bits_h=bits, vec8_h=vec8, soft={})
    return _STATE["rig"]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for k in ("rig", "mem"):
        if k in _STATE:
            _STATE.pop(k)["b"].close()
    _STATE.clear()


def _soft(tau, w_ptr=None):
    """The 9-row call at temperature tau with the probes and the heat map (under synthetic(7): one call per tau for the
    module; another blob's call is not kept)."""
    r = _rig()
    call = lambda w: r["b"].policy_forward_obs_soft(w, NOBS, r["bits"].ptr, r["vec8"].ptr, tau, want_probe_ptr=r["probe"].ptr,
                                                    want_heat=True)
    if w_ptr is not None:
        return call(w_ptr)
    if tau not in r["soft"]:
        r["soft"][tau] = call(r["w"].ptr)
    return r["soft"][tau]


def _check_against_float64(out, tau, tag, worst):
    """The bounds of the accuracy contract on one call's outputs, against the float64 reduction of its own heat map."""
    ref_soft, ref_mass = so.soft_rows(out["heat"], tau)
    for k in range(len(ref_soft)):
        assert out["ptr_max"][k] == out["heat"][k].max(), (tag, k)
        e_mass = abs(float(out["ptr_mass"][k]) - ref_mass[k]) / ref_mass[k]
        e_soft = abs(float(out["ptr_soft"][k]) - ref_soft[k])
        ulp4 = 4.0 * float(np.spacing(np.float32(abs(ref_soft[k]))))
        worst["mass"] = max(worst["mass"], e_mass)
        worst["soft"] = max(worst["soft"], max(0.0, e_soft - ulp4) / tau)
        worst["ulps"] = max(worst.get("ulps", 0.0), 4.0 * e_soft / ulp4)
        print("%s tau %-6g row %d: mass %.9g (ref %.9g, rel err %.2e)  soft %.9g (ref %.9g, err %.2e = %.2e T, 4 ulp %.1e)"
              % (tag, tau, k, out["ptr_mass"][k], ref_mass[k], e_mass, out["ptr_soft"][k], ref_soft[k], e_soft, e_soft / tau, ulp4))
        assert e_mass <= so.mass_bound(), (tag, tau, k, e_mass)
        assert e_soft <= so.soft_bound(tau, ref_soft[k]), (tag, tau, k, e_soft)
    return ref_soft, ref_mass


# ------------------------------------------------------------------------------ 1. where it must be ofx_policy_forward_obs
def test_temperature_zero_is_the_maximum_and_shared_outputs_are_forward_obs():
    r = _rig()
    plain = r["b"].policy_forward_obs(r["w"].ptr, NOBS, r["bits"].ptr, r["vec8"].ptr, want_probe_ptr=r["probe"].ptr)
    zero = _soft(0.0)
    assert np.isfinite(zero["ptr_max"]).all()
    assert zero["ptr_soft"].tobytes() == zero["ptr_max"].tobytes()
    assert (zero["ptr_mass"] == 1.0).all()
    for tau in (0.0, 0.3):
        out = _soft(tau)
        for k in SHARED:
            assert out[k].tobytes() == plain[k].tobytes(), (tau, k)
    for k in range(NOBS):                                                # the probes read the map that was summed
        x, y = PROBES[k]
        assert _soft(0.3)["ptr_probe"][k] == _soft(0.3)["heat"][k, y, x]
    assert _soft(0.3)["heat"].tobytes() == zero["heat"].tobytes()


# ------------------------------------------------------------------------------ 2. every pixel once
def test_every_pixel_counts_once():
    """At T = 1e30 every term is exactly 1: a pixel that is missed, doubled or read from an idle lane - at the seam of a
    ship's two workgroups, on the frame - changes the count."""
    out = _soft(1e30)
    print("ptr_mass at T = 1e30:", out["ptr_mass"].tolist())
    assert (out["ptr_mass"] == 160000.0).all()
    lean = _rig()["b"].policy_forward_obs_soft(_rig()["w"].ptr, NOBS, _rig()["bits"].ptr, _rig()["vec8"].ptr, 1e30)
    assert (lean["ptr_mass"] == 160000.0).all()                         # and without the heat map / probe (EXTRA = false)
    assert lean["ptr_soft"].tobytes() == out["ptr_soft"].tobytes()


# ------------------------------------------------------------------------------ 3. against float64
def test_against_float64_on_the_calls_own_heat_map():
    worst = dict(mass=0.0, soft=0.0)
    for tau in TAUS:
        ref_soft, ref_mass = _check_against_float64(_soft(tau), tau, "synthetic(7)", worst)
        if tau in (0.3, 1.0):                                            # not passing on the maximum alone
            assert (ref_mass >= 1000.0).all(), (tau, ref_mass.tolist())
    lean = _rig()["b"].policy_forward_obs_soft(_rig()["w"].ptr, NOBS, _rig()["bits"].ptr, _rig()["vec8"].ptr, 0.3)
    assert lean["ptr_soft"].tobytes() == _soft(0.3)["ptr_soft"].tobytes()       # EXTRA = false: the same sum
    assert lean["ptr_mass"].tobytes() == _soft(0.3)["ptr_mass"].tobytes()
    print("test 3: largest relative error of ptr_mass %.3e (allowed %.3e), largest error of ptr_soft behind 4 ulp %.3e T "
          "(allowed %.3e T), largest error of ptr_soft %.2f ulp(ref)"
          % (worst["mass"], so.mass_bound(), worst["soft"], min(2 * so.SOFT_T_ERR, so.SOFT_T_CONTRACT), worst["ulps"]))


# ------------------------------------------------------------------------------ 4. the frame
def test_leading_term_on_the_frame():
    from ofighters_amd import DeviceBuffer
    worst = dict(mass=0.0, soft=0.0)
    seen = set()
    for ci, case in enumerate(CASES):
        w = frame_weights(case, 40 + ci)
        w_d = DeviceBuffer(w.nbytes).upload(w)
        out = _soft(0.03, w_d.ptr)
        for k in range(NOBS):
            y, x = divmod(int(np.argmax(out["heat"][k])), W)
            assert case in where(y, x), "the weights of case %r did not put the maximum there: row %d (y %d, x %d)" % (case, k, y, x)
            assert tuple(out["ipointer"][k]) == (x, y)
            seen.update(where(y, x))
        _check_against_float64(out, 0.03, case, worst)
        _rig()["b"].sync()
        w_d.free()
    assert seen >= set(CASES), seen
    print("test 4: largest relative error of ptr_mass %.3e, largest error of ptr_soft behind 4 ulp %.3e T, largest error of ptr_soft "
          "%.2f ulp(ref)" % (worst["mass"], worst["soft"], worst["ulps"]))


# ------------------------------------------------------------------------------ 5. rows are independent
def test_rows_do_not_depend_on_the_batch():
    r = _rig()
    words = 2 * W * H // 32
    whole = _soft(0.3)
    for k in range(NOBS):
        one = r["b"].policy_forward_obs_soft(r["w"].ptr, 1, r["bits"].ptr + 4 * words * k, r["vec8"].ptr + 32 * k, 0.3,
                                             want_probe_ptr=r["probe"].ptr + 8 * k, want_heat=True)
        for name in SHARED + ("ptr_soft", "ptr_mass", "heat"):
            assert one[name][0].tobytes() == whole[name][k].tobytes(), (k, name)


# ------------------------------------------------------------------------------ 6. ofx_dqn_targets_soft
NM, MM, CAPM, SEEDM, GAMMA = 32, 6, 50, 0x0F160521, 0.9
NROWS = 9


def _memory():
    """32 arenas x 6 ships, capacity 50, 120 lock-steps of random play captured for three ships (episodes restart inside
    the memory); 9 gathered transitions around the first sampled row with done != 0, one-step and as 3-step windows."""
    if "mem" in _STATE:
        return _STATE["mem"]
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    b = ArenaBatch(NM, MM)
    b.replay_create(CAPM, 0)
    b.spawn_random(SEEDM)
    mask = np.zeros((NM, MM), np.uint8)
    mask[:, [0, 2, 5]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * NM * MM), DeviceBuffer(8 * NM * MM)
    for t in range(120):
        if (t + 40) % 60 == 0:
            b.restart_random(SEEDM)
        b.bot_actions(["random"] * MM, SEEDM, tick=t)
        b.policy_explore(1.0, SEEDM, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    slot, n_s = b.replay_sample(SEEDM, 0, CAPM)
    b.sync()
    slot_h, n_h = slot.download(np.int32, (NM, CAPM)), n_s.download(np.int32, (NM,))
    entries = [(a, int(slot_h[a, j])) for a in range(NM) for j in range(n_h[a])]
    mem = [b.replay_rows(a) for a in range(NM)]
    first = max(0, next(k for k, (a, s) in enumerate(entries) if mem[a][s]["done"]) - 4)
    words = W * H // 32
    w = synthetic(7)
    st = dict(b=b, w=DeviceBuffer(w.nbytes).upload(w))
    for name, nstep in (("one", None), ("nstep", 3)):
        g = dict(rows=DeviceBuffer(NROWS * b.TRANSITION_DTYPE.itemsize), bp=DeviceBuffer(4 * NROWS * 2 * words),
                 bn=DeviceBuffer(4 * NROWS * 2 * words), ret=None, disc=None)
        if nstep is None:
            got = b.replay_gather_valid_into(slot, n_s, CAPM, first, NROWS, g["rows"], g["bp"], g["bn"])
        else:
            g["ret"], g["disc"] = DeviceBuffer(4 * NROWS), DeviceBuffer(4 * NROWS)
            got = b.replay_gather_nstep_into(slot, n_s, CAPM, first, NROWS, nstep, GAMMA, g["rows"], g["bp"], g["bn"], g["ret"],
                                             g["disc"])
        assert got == NROWS
        b.sync()
        g["host"] = g["rows"].download(b.TRANSITION_DTYPE, (NROWS,))
        if nstep is not None:
            g["ret_h"], g["disc_h"] = g["ret"].download(np.float32, (NROWS,)), g["disc"].download(np.float32, (NROWS,))
        st[name] = g
    # the padded variant: the one-step window with row 2 made a padding row
    pad = dict(st["one"])
    host = st["one"]["host"].copy()
    host["ship"][2] = -1
    pad["rows"], pad["host"] = DeviceBuffer(host.nbytes).upload(host), host
    st["padded"] = pad
    _STATE["mem"] = st
    return st


def _ptr(x):
    return x.ptr if x is not None else None


def _targets_soft(st, g, tau, alpha=0.0, clip=0.0, current=True):
    from ofighters_amd import DeviceBuffer
    out = [DeviceBuffer(4 * NROWS) if (current or k >= 2) else None for k in range(4)]
    st["b"].dqn_targets_soft_into(st["w"].ptr, NROWS, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA, out[2].ptr, out[3].ptr,
                                  tau[0], tau[1], alpha, clip, _ptr(g["ret"]), _ptr(g["disc"]), _ptr(out[0]), _ptr(out[1]))
    st["b"].sync()
    return [o.download(np.float32, (NROWS,)) if o else None for o in out]


def _targets_plain(st, g):
    from ofighters_amd import DeviceBuffer, _native as nat
    out = [DeviceBuffer(4 * NROWS) for _ in range(4)]
    L, b = nat.lib(), st["b"]
    if g["ret"] is None:
        nat.check(L.ofx_dqn_targets(b.handle, st["w"].ptr, NROWS, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA, *[o.ptr for o in out]))
    else:
        nat.check(L.ofx_dqn_targets_nstep(b.handle, st["w"].ptr, NROWS, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, g["ret"].ptr,
                                          g["disc"].ptr, *[o.ptr for o in out]))
    b.sync()
    return [o.download(np.float32, (NROWS,)) for o in out]


def _forwards(st, g, tau_ptr):
    """ofx_policy_forward_obs_soft on the window's two map sets: what the targets kernel saw (the library is reproducible
    to the bit)."""
    from ofighters_amd import DeviceBuffer
    b, host = st["b"], g["host"]
    probe = np.stack([np.clip(host["px"], 0, W - 1), np.clip(host["py"], 0, H - 1)], axis=1).astype(np.int32)
    probe_d = DeviceBuffer(probe.nbytes).upload(probe)
    pad = host["ship"] < 0
    vp = np.where(pad[:, None], np.float32(0), np.ascontiguousarray(host["head_prev"], np.float32))
    vn = np.where(pad[:, None], np.float32(0), np.ascontiguousarray(host["head_next"], np.float32))
    vp_d, vn_d = DeviceBuffer(vp.nbytes).upload(np.ascontiguousarray(vp)), DeviceBuffer(vn.nbytes).upload(np.ascontiguousarray(vn))
    prev = b.policy_forward_obs_soft(st["w"].ptr, NROWS, g["bp"].ptr, vp_d.ptr, tau_ptr, want_probe_ptr=probe_d.ptr)
    nxt = b.policy_forward_obs_soft(st["w"].ptr, NROWS, g["bn"].ptr, vn_d.ptr, tau_ptr)
    return prev, nxt


@pytest.mark.parametrize("window", ["one", "nstep", "padded"])
def test_targets_at_temperature_zero_are_the_plain_targets(window):
    st = _memory()
    g = st[window]
    assert 0 < (g["host"]["done"] != 0).sum() < NROWS
    plain, soft = _targets_plain(st, g), _targets_soft(st, g, (0.0, 0.0))
    for k, name in enumerate(("q_sa", "p_sp", "y_act", "y_ptr")):
        assert np.isfinite(plain[k]).all(), name
        assert soft[k].tobytes() == plain[k].tobytes(), (window, name)
    lean = _targets_soft(st, g, (0.0, 0.0), current=False)
    assert lean[2].tobytes() == plain[2].tobytes() and lean[3].tobytes() == plain[3].tobytes()
    if window == "padded":
        assert all(o[2] == 0.0 for o in soft) and (soft[2][[0, 1, 3]] != 0).any()


@pytest.mark.parametrize("window", ["one", "nstep", "padded"])
def test_soft_targets_against_float64(window):
    st = _memory()
    g = st[window]
    tau = (0.5, 0.3)
    q_sa, p_sp, y_act, y_ptr = _targets_soft(st, g, tau)
    prev, nxt = _forwards(st, g, tau[1])
    ret, disc = (g["ret_h"], g["disc_h"]) if window == "nstep" else (None, None)
    want_act, want_ptr = so.targets(g["host"], GAMMA, ret, disc, tau[0], nxt["act"], nxt["ptr_soft"])
    real = g["host"]["ship"] >= 0
    for got, want, v, name in ((y_act, want_act, so.soft_act(nxt["act"], tau[0]), "y_act"), (y_ptr, want_ptr, nxt["ptr_soft"], "y_ptr")):
        err, bound = np.abs(got.astype(np.float64) - want), so.target_bound(g["host"], 0.0, 0.0, v, ret)
        print("%s %s: largest error %.3e, smallest bound %.3e" % (window, name, err.max(), bound.min()))
        assert (err <= bound).all(), (window, name, err.tolist(), bound.tolist())
        assert (got[~real] == 0).all()
    assert q_sa[real].tobytes() == prev["act"][np.arange(NROWS), (g["host"]["iaction"] != 0).astype(int)][real].tobytes()
    assert p_sp[real].tobytes() == prev["ptr_probe"][real].tobytes()
    # the soft value is above the maximum where the row bootstraps: these are not the plain targets
    plain = _targets_plain(st, g)
    boot = real & ((g["disc_h"] != 0) if window == "nstep" else (g["host"]["done"] == 0))
    assert boot.any() and (y_ptr[boot] > plain[3][boot]).all() and (y_act[boot] >= plain[2][boot]).all()
    assert y_ptr[real & ~boot].tobytes() == plain[3][real & ~boot].tobytes()
    lean = _targets_soft(st, g, tau, current=False)
    assert lean[2].tobytes() == y_act.tobytes() and lean[3].tobytes() == y_ptr.tobytes()


# (tau, alpha, clip): the issue's setting, where on these rows every term sits on one of its two ends (the action values
# are about 22 apart, so T ln pi is 0 or -22 at tau_act 0.5, and every probed pixel lies more than 1 below the soft
# value) - and a setting that puts rows strictly between the ends on both heads, where the term is alpha * (q - V(state))
# itself: the value of V(state), the probe and the chosen action's value all enter the result
MUNCHAUSEN = [((0.5, 0.3), 0.9, -1.0), ((10.0, 0.3), 0.9, -10.0)]


@pytest.mark.parametrize("tau,alpha,clip", MUNCHAUSEN, ids=["saturated", "linear"])
@pytest.mark.parametrize("window", ["one", "padded"])
def test_munchausen_targets_against_float64(window, tau, alpha, clip):
    st = _memory()
    g = st[window]
    q_sa, p_sp, y_act, y_ptr = _targets_soft(st, g, tau, alpha, clip)
    prev, nxt = _forwards(st, g, tau[1])
    kw = dict(alpha=alpha, clip=clip, act_prev=prev["act"], probe_prev=prev["ptr_probe"], soft_prev=prev["ptr_soft"])
    want_act, want_ptr = so.targets(g["host"], GAMMA, None, None, tau[0], nxt["act"], nxt["ptr_soft"], **kw)
    real = g["host"]["ship"] >= 0
    for got, want, v, name in ((y_act, want_act, so.soft_act(nxt["act"], tau[0]), "y_act"), (y_ptr, want_ptr, nxt["ptr_soft"], "y_ptr")):
        err, bound = np.abs(got.astype(np.float64) - want), so.target_bound(g["host"], alpha, clip, v)
        print("%s %s: largest error %.3e, smallest bound %.3e" % (window, name, err.max(), bound.min()))
        assert (err <= bound).all(), (window, name, err.tolist(), bound.tolist())
        assert (got[~real] == 0).all()
    # the log-policy terms: at least one row is clipped and one is not
    ia = (g["host"]["iaction"] != 0).astype(int)
    l_act = prev["act"][np.arange(NROWS), ia].astype(np.float64) - so.soft_act(prev["act"], tau[0])
    l_ptr = prev["ptr_probe"].astype(np.float64) - prev["ptr_soft"].astype(np.float64)
    l = np.concatenate([l_act[real], l_ptr[real]])
    print("%s clip %g: T ln pi per head %s / %s" % (window, clip, np.round(l_act, 3).tolist(), np.round(l_ptr, 3).tolist()))
    assert (l < clip).any() and (l > clip).any()
    if clip == -10.0:   # rows strictly inside (clip, 0) on BOTH heads, next to a clipped one: the linear branch is compared
        for name, lh in (("action", l_act[real]), ("pointer", l_ptr[real])):
            assert ((lh > clip + 1e-3) & (lh < -1e-3)).any(), (name, lh.tolist())
        # and the result depends on V(state) there: the same rows with the other setting's term differ by more than the bound
        inside = real & (l_ptr > clip + 1e-3) & (l_ptr < -1e-3)
        assert (np.abs(want_ptr[inside] - so.targets(g["host"], GAMMA, None, None, tau[0], nxt["act"], nxt["ptr_soft"],
                                                     **dict(kw, soft_prev=prev["ptr_soft"] + np.float32(0.01)))[1][inside])
                > 10 * so.target_bound(g["host"], alpha, clip, nxt["ptr_soft"])[inside]).all()
    # the same call without q_sa / p_sp still runs the forward on `state`
    lean = _targets_soft(st, g, tau, alpha, clip, current=False)
    assert lean[2].tobytes() == y_act.tobytes() and lean[3].tobytes() == y_ptr.tobytes()
    soft_only = _targets_soft(st, g, tau)
    assert (y_act[real] <= soft_only[2][real]).all() and (y_ptr[real] < soft_only[3][real]).any()
    assert q_sa.tobytes() == soft_only[0].tobytes() and p_sp.tobytes() == soft_only[1].tobytes()


def test_invalid_arguments_write_nothing():
    from ofighters_amd import DeviceBuffer, _native as nat
    st = _memory()
    b, L, g, gn = st["b"], nat.lib(), st["one"], st["nstep"]
    mark = np.full(NROWS, -77.5, np.float32)
    out = [DeviceBuffer(4 * NROWS).upload(mark) for _ in range(4)]
    nan, inf = float("nan"), float("inf")

    def call(tau_act=0.5, tau_ptr=0.3, alpha=0.0, clip=0.0, ret=None, disc=None, w=st["w"], outs=out):
        return L.ofx_dqn_targets_soft(b.handle, _ptr(w), NROWS, g["rows"].ptr, g["bp"].ptr, g["bn"].ptr, GAMMA, _ptr(ret), _ptr(disc),
                                      tau_act, tau_ptr, alpha, clip, *[_ptr(o) for o in outs])
    for bad in (-1.0, nan, inf, 1e-7, 1e31):
        assert call(tau_act=bad) == nat.OFX_ERR_INVALID, bad
        assert call(tau_ptr=bad) == nat.OFX_ERR_INVALID, bad
    for bad in (-0.1, 1.5, nan, inf):
        assert call(alpha=bad, clip=-1.0) == nat.OFX_ERR_INVALID, bad
    for bad in (0.5, nan, -inf, inf):
        assert call(alpha=0.9, clip=bad) == nat.OFX_ERR_INVALID, bad
    assert call(alpha=0.9, clip=-1.0, tau_act=0.0) == nat.OFX_ERR_INVALID          # Munchausen needs both taus > 0
    assert call(alpha=0.9, clip=-1.0, tau_ptr=0.0) == nat.OFX_ERR_INVALID
    assert call(alpha=0.9, clip=-1.0, ret=gn["ret"], disc=gn["disc"]) == nat.OFX_ERR_INVALID   # and the one-step form
    assert call(ret=gn["ret"]) == nat.OFX_ERR_INVALID and call(disc=gn["disc"]) == nat.OFX_ERR_INVALID
    assert call(w=None) == nat.OFX_ERR_INVALID
    assert call(outs=[out[0], None, out[2], out[3]]) == nat.OFX_ERR_INVALID       # q_sa without p_sp
    assert call(outs=[None, None, None, out[3]]) == nat.OFX_ERR_INVALID
    r = _rig()
    soft_d, mass_d = DeviceBuffer(4 * NOBS).upload(mark), DeviceBuffer(4 * NOBS).upload(mark)
    for bad in (-1.0, nan, inf, 1e-7, 1e31):
        rc = L.ofx_policy_forward_obs_soft(r["b"].handle, r["w"].ptr, NOBS, r["bits"].ptr, r["vec8"].ptr, bad, None, None, None, None,
                                           None, None, soft_d.ptr, mass_d.ptr, None)
        assert rc == nat.OFX_ERR_INVALID, bad
    b.sync(), r["b"].sync()
    for o in out + [soft_d, mass_d]:
        assert o.download(np.float32, (NROWS,)).tobytes() == mark.tobytes()
    # and the valid calls next to them pass
    assert call() == nat.OFX_OK and call(alpha=0.9, clip=-1.0) == nat.OFX_OK and call(alpha=1.0, clip=0.0) == nat.OFX_OK
    assert call(tau_act=1e-6, tau_ptr=1e30) == nat.OFX_OK
    b.sync()
    assert all(np.isfinite(o.download(np.float32, (NROWS,))).all() for o in out)


# ------------------------------------------------------------------------------ 7. the trainer, with a checkpoint
N7, M7, STEPS7, SEED7 = 3, 2, 8, 0x0F160B21


def _build7(**kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(N7, M7)
    eps = Epsilon_decay()
    eps.set(0.9)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=4, memory_size=16, fit_batch=8, **kw)
    roll = TrainingRollout(b, tr, ["random"] * M7, SEED7, policy_ships=(0, 1), episode_ticks=20, collecting_steps=2,
                           replay_every=2, replay_on_death=False)
    return b, tr, roll


def _state7(b, tr):
    b.sync()
    tgt = tr.target_host()
    return dict(weights=tr.weights_host().tobytes(), target=None if tgt is None else tgt.tobytes(),
                rows=[b.replay_rows(g).tobytes() for g in range(b.N)], fit_steps=tr.fit_steps)


def test_trainer_soft_targets_off_at_zero_and_on_otherwise():
    end = {}
    for name, kw in (("default", dict()), ("zero", dict(soft_targets=(0.0, 0.0))), ("soft", dict(soft_targets=(0.5, 0.3)))):
        b, tr, roll = _build7(**kw)
        roll.run(STEPS7)
        end[name] = _state7(b, tr)
        assert np.isfinite(np.array(tr.losses)).all() and tr.fit_steps >= 3
        assert ("soft_targets" in tr.fingerprint()) == (name != "default")
        b.close()
    assert end["zero"]["weights"] == end["default"]["weights"] and end["zero"]["fit_steps"] == end["default"]["fit_steps"]
    assert end["soft"]["weights"] != end["default"]["weights"] and end["soft"]["fit_steps"] == end["default"]["fit_steps"]
    assert end["soft"]["rows"] == end["default"]["rows"]                 # what was played and stored does not change


def test_munchausen_rollout_resumes_bit_for_bit(tmp_path):
    kw = dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0), target_sync=3, prioritized=True)
    b, tr, roll = _build7(**kw)
    path = str(tmp_path / "ck")
    roll.run(4)
    mid = _state7(b, tr)
    roll.checkpoint(path)
    roll.run(STEPS7 - 4)
    end = _state7(b, tr)
    assert tr.fit_steps >= 3 and end["weights"] != mid["weights"] and end["target"] != end["weights"]
    b.close()
    del b, tr, roll
    b, tr, roll = _build7(**kw)
    man = roll.restore(path)
    assert man["trainer_fingerprint"]["soft_targets"] == [0.5, 0.3] and man["trainer_fingerprint"]["munchausen"] == [0.9, -1.0]
    after = _state7(b, tr)
    assert [k for k in after if after[k] != mid[k]] == []
    roll.run(STEPS7 - 4)
    got = _state7(b, tr)
    assert [k for k in got if got[k] != end[k]] == []
    b.close()
    # the Munchausen term did something: the same run without it ends elsewhere
    b, tr, roll = _build7(**dict(kw, munchausen=None))
    roll.run(STEPS7)
    assert _state7(b, tr)["weights"] != end["weights"]
    b.close()
