"""Soft (entropy-regularised) and Munchausen targets without a GPU (include/ofx.h, "soft and Munchausen targets"): the two
symbols, the float64 restatement of tests/soft_oracle.py on hand-built arrays, and DeviceTrainer's two options on the
recording stand-ins of tests/replay_standin.py - what is refused before any device call, what the option changes in the
call log, and the fingerprint."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import replay_standin as st
from tests import soft_oracle as so

SOFT_SYMBOLS = ["ofx_policy_forward_obs_soft", "ofx_dqn_targets_soft"]


def test_soft_symbols_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in SOFT_SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    assert len(nat.SIGNATURES["ofx_policy_forward_obs_soft"][1]) == 15 and len(nat.SIGNATURES["ofx_dqn_targets_soft"][1]) == 17


# ---- the restatement -----------------------------------------------------------------------------------------------
def _rows(reward, done, ship=None, iaction=None):
    from ofighters_amd.engine import ArenaBatch
    rows = np.zeros(len(reward), ArenaBatch.TRANSITION_DTYPE)
    rows["reward"], rows["done"] = reward, done
    rows["ship"] = 0 if ship is None else ship
    rows["iaction"] = 0 if iaction is None else iaction
    return rows


def test_lse_tends_to_the_maximum_and_counts_uniform_values():
    rs = np.random.RandomState(3)
    v = rs.normal(size=(40, 50)).astype(np.float32)
    prev = math.inf
    for T in (1.0, 0.1, 1e-2, 1e-3, 1e-6):
        soft, mass, m = so.lse(v, T)
        assert m == v.max() and soft >= m and soft - m <= T * math.log(v.size) and soft - m <= prev
        assert soft - m < prev or soft == m                     # strictly nearer, until it is the maximum itself
        prev = soft - m
    assert so.lse(v, 1e-6)[0] == v.max() and so.lse(v, 1e-6)[1] == 1.0
    for T in (0.03, 1.0, 1e30):                                 # n equal values: max + T ln n, mass n
        soft, mass, m = so.lse(np.full((7, 11), -2.5, np.float32), T)
        assert mass == 77.0 and soft == -2.5 + T * math.log(77.0)
    soft, mass = so.soft_rows(v[None], 0)                       # T == 0: the maximum itself, mass 1
    assert soft[0] == v.max() and mass[0] == 1.0
    a = np.array([[1.0, 3.0], [2.0, 2.0], [-1.0, -4.0]], np.float32)
    assert so.soft_act(a, 0).tolist() == [3.0, 2.0, -1.0]
    got = so.soft_act(a, 0.5)
    assert np.allclose(got, [so.lse(r, 0.5)[0] for r in a], rtol=0, atol=1e-15) and got[1] == 2.0 + 0.5 * math.log(2.0)


def test_munchausen_term_is_zero_when_deterministic_and_alpha_clip_when_clipped():
    # a policy that puts all its mass on the action taken: q == V(state), the term is 0
    assert so.munchausen_term(1.25, 1.25, 0.9, -1.0) == 0.0
    # ln pi far below the clip: alpha * clip
    assert so.munchausen_term(-7.0, 2.0, 0.9, -1.0) == 0.9 * -1.0
    # in between: alpha * (q - V); a rounding that leaves q above V gives 0, never a bonus
    assert so.munchausen_term(1.0, 1.5, 0.5, -1.0) == -0.25 and so.munchausen_term(1.5 + 1e-9, 1.5, 0.5, -1.0) == 0.0
    act_prev = np.array([[40.0, -40.0], [40.0, -40.0]], np.float32)      # softmax(act / 0.5) is deterministic on action 0
    rows = _rows([2, 2], [1, 1], iaction=[0, 1])
    y_act, y_ptr = so.targets(rows, 0.9, None, None, 0.5, np.zeros((2, 2), np.float32), np.zeros(2), alpha=0.9, clip=-1.0,
                              act_prev=act_prev, probe_prev=[3.0, -9.0], soft_prev=[3.0, 3.0])
    assert y_act.tolist() == [2.0, 2.0 - 0.9] and y_ptr.tolist() == [2.0, 2.0 - 0.9]


def test_done_padding_and_nstep_rows():
    act_next = np.array([[0.5, 1.5], [2.0, -1.0], [0.25, 0.25], [4.0, 1.0]], np.float32)
    soft_next = np.array([3.0, 5.0, 7.0, 9.0])
    rows = _rows([3, -2, 1, 4], [0, 1, 0, 0], ship=[0, 1, -1, 2], iaction=[1, 0, 0, 1])
    kw = dict(alpha=0.5, clip=-2.0, act_prev=np.array([[1.0, 0.0]] * 4, np.float32), probe_prev=[0.0, 0.5, 1.0, -8.0],
              soft_prev=[1.0, 1.0, 1.0, 1.0])
    y_act, y_ptr = so.targets(rows, 0.9, None, None, 0.5, act_next, soft_next, **kw)
    v_prev = so.soft_act(kw["act_prev"], 0.5)
    # a done row: the reward plus the Munchausen term alone
    assert y_act[1] == -2.0 + 0.5 * max(1.0 - v_prev[1], -2.0) and y_ptr[1] == -2.0 + 0.5 * (0.5 - 1.0)
    # a padding row: zeros
    assert y_act[2] == 0.0 and y_ptr[2] == 0.0
    # a live row: both parts; the pointer head's term is clipped (-8 - 1 < -2)
    assert y_ptr[3] == 4.0 + 0.5 * -2.0 + 0.9 * 9.0
    assert y_act[0] == 3.0 + 0.5 * (0.0 - v_prev[0]) + 0.9 * so.soft_act(act_next[:1], 0.5)[0]
    # alpha == 0 and tau == 0: the hard targets
    h_act, h_ptr = so.targets(rows, 0.9, None, None, 0.0, act_next, soft_next)
    assert h_act.tolist() == [3.0 + 0.9 * 1.5, -2.0, 0.0, 4.0 + 0.9 * 4.0] and h_ptr[0] == 3.0 + 0.9 * 3.0
    # the n-step form ignores gamma (and the rows' rewards and done flags)
    ret, disc = np.array([1.0, 2.0, 3.0, 4.0]), np.array([0.5, 0.0, 0.25, 0.125])
    a1, p1 = so.targets(rows, 0.9, ret, disc, 0.5, act_next, soft_next)
    a2, p2 = so.targets(rows, 0.1, ret, disc, 0.5, act_next, soft_next)
    assert a1.tobytes() == a2.tobytes() and p1.tobytes() == p2.tobytes()
    assert p1.tolist() == [1.0 + 0.5 * 3.0, 2.0, 0.0, 4.0 + 0.125 * 9.0]
    with pytest.raises(ValueError):
        so.targets(rows, 0.9, ret, None, 0.5, act_next, soft_next)
    with pytest.raises(ValueError):
        so.targets(rows, 0.9, ret, disc, 0.5, act_next, soft_next, **kw)


def test_bounds_never_exceed_the_contract():
    assert so.mass_bound() <= so.MASS_REL_CONTRACT == 1e-4 and so.mass_bound() == min(2 * so.MASS_REL_ERR, 1e-4)
    ref = np.array([1.0, -3.0])
    b = so.soft_bound(0.3, ref)
    assert (b <= 1e-4 * 0.3 + 4 * np.spacing(np.abs(ref).astype(np.float32))).all()
    rows = _rows([3, -20], [0, 0])
    assert so.target_bound(rows, 0.9, -1.0, [0.5, -4.0]).tolist() == [2e-6 * 4.4, 2e-6 * 24.9]


def test_observations_are_nine_distinct_maps_with_a_corner_disc():
    bits, vec8 = so.observations()
    assert bits.shape == (9, 2, 5000) and bits.dtype == np.uint32 and vec8.shape == (9, 8) and vec8.dtype == np.float32
    maps = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(9, 2, 400, 400)     # bit p & 31 of word p >> 5
    assert len({m.tobytes() for m in maps}) == 9
    for k in range(9):
        assert maps[k, 0].sum() > 900 and maps[k, 1].sum() > 50
        cy, cx = [(0, 0), (0, 399), (399, 0), (399, 399)][k % 4]
        assert maps[k, 0, cy, cx] == 1                                                        # the disc covers the corner pixel


# ---- DeviceTrainer(soft_targets=, munchausen=) -----------------------------------------------------------------------
class SoftRecordingBatch(st.RecordingBatch):
    """The recording stand-in with the one call the option adds."""

    def dqn_targets_soft_into(self, w, n, rows_p, prev_p, next_p, gamma, y_act_p, y_ptr_p, tau_act, tau_ptr, m_alpha=0.0,
                              m_clip=0.0, ret_p=None, disc_p=None, q_sa_p=None, p_sp_p=None):
        self._log("ofx_dqn_targets_soft", (w, n, rows_p, prev_p, next_p, float(gamma), ret_p, disc_p, tau_act, tau_ptr, m_alpha,
                                            m_clip, q_sa_p, p_sp_p, y_act_p, y_ptr_p))


def _trainer(monkeypatch, **kw):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch = SoftRecordingBatch()
    t = tr.DeviceTrainer(batch, np.arange(st.N_FLOATS, dtype=np.float32), **dict(st.COMMON, **kw))
    batch.trainer = t
    return batch, t


def _replays(monkeypatch, sched, **kw):
    batch, t = _trainer(monkeypatch, **kw)
    out = {"setup": list(batch.log), "replays": []}
    for step in sched:
        del batch.log[:]
        batch.step = step
        t.replay()
        out["replays"].append({"log": list(batch.log), "losses": list(t.losses),
                               "scratch": {k: b.nbytes for k, b in sorted(t._buf.items())}})
    return out


PAIR_BAD = [1.0, (1.0,), (1.0, 2.0, 3.0), (float("nan"), 1.0), (1.0, float("inf")), ("1", 1.0), (True, 1.0), (None, 1.0), "ab"]
SOFT_BAD = PAIR_BAD + [(-1.0, 1.0), (1.0, -0.5), (1e-7, 1.0), (1.0, 1e31)]
MUNCH_BAD = PAIR_BAD + [(-0.1, -1.0), (1.5, -1.0), (0.9, 0.5)]


@pytest.mark.parametrize("bad", SOFT_BAD, ids=[repr(b) for b in SOFT_BAD])
def test_bad_soft_targets_are_refused_before_any_device_call(monkeypatch, bad):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch, made = SoftRecordingBatch(), st.HostBuffer.count
    with pytest.raises(ValueError, match="soft_targets"):
        tr.DeviceTrainer(batch, np.zeros(4, np.float32), soft_targets=bad)
    assert batch.log == [] and st.HostBuffer.count == made


@pytest.mark.parametrize("bad", MUNCH_BAD, ids=[repr(b) for b in MUNCH_BAD])
def test_bad_munchausen_is_refused_before_any_device_call(monkeypatch, bad):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch, made = SoftRecordingBatch(), st.HostBuffer.count
    with pytest.raises(ValueError, match="munchausen"):
        tr.DeviceTrainer(batch, np.zeros(4, np.float32), soft_targets=(0.5, 0.3), munchausen=bad)
    assert batch.log == [] and st.HostBuffer.count == made


REFUSED = [("munchausen", dict(munchausen=(0.9, -1.0))),                                       # without soft_targets
           ("munchausen", dict(munchausen=(0.9, -1.0), soft_targets=(0.0, 0.3))),              # a tau that is 0
           ("munchausen", dict(munchausen=(0.9, -1.0), soft_targets=(0.5, 0.0))),
           ("munchausen", dict(munchausen=(0.9, -1.0), soft_targets=(0.5, 0.3), n_step=3)),
           ("soft_targets", dict(soft_targets=(0.5, 0.3), double_dqn=True)),
           ("soft_targets", dict(soft_targets=(0.5, 0.3), double_dqn=True, target_sync=2)),
           ("soft_targets", dict(soft_targets=(0.5, 0.3), reference_quirks=True)),
           ("soft_targets|munchausen", dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0), double_dqn=True)),
           ("soft_targets|munchausen", dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0), reference_quirks=True))]


@pytest.mark.parametrize("match,kw", REFUSED, ids=[repr(k) for _, k in REFUSED])
def test_refused_combinations(monkeypatch, match, kw):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch, made = SoftRecordingBatch(), st.HostBuffer.count
    with pytest.raises(ValueError, match=match):
        tr.DeviceTrainer(batch, np.zeros(4, np.float32), **kw)
    assert batch.log == [] and st.HostBuffer.count == made


def test_good_arguments_become_pairs_of_floats(monkeypatch):
    for arg, want in (((0, 0), (0.0, 0.0)), ([0.5, 2], (0.5, 2.0)), (np.array([1.5, 0.25], np.float32), (1.5, 0.25)),
                      ((1e-6, 1e30), (1e-6, 1e30))):
        t = _trainer(monkeypatch, soft_targets=arg)[1]
        assert t.soft_targets == want and all(type(v) is float for v in t.soft_targets) and t.munchausen is None
    t = _trainer(monkeypatch, soft_targets=(0.5, 0.3), munchausen=[1, -2])[1]
    assert t.munchausen == (1.0, -2.0)
    t = _trainer(monkeypatch)[1]
    assert t.soft_targets is None and t.munchausen is None


OPTIONS = [dict(), dict(prioritized=True), dict(n_step=3), dict(target_sync=2), dict(huber_delta=1.0, clip_norm=10.0),
           dict(global_sampling=True), dict(global_sampling=True, accumulate=2, prioritized=True),
           dict(prioritized=True, actor_priorities=True), dict(packed_memory=True)]


@pytest.mark.parametrize("kw", OPTIONS, ids=[repr(k) for k in OPTIONS])
def test_soft_targets_replace_the_plain_targets_call_and_nothing_else(monkeypatch, kw):
    """The log with soft_targets set is the log without it with every ofx_dqn_targets / ofx_dqn_targets_nstep entry
    replaced by one ofx_dqn_targets_soft on the same blob, rows, maps, returns and outputs."""
    sched = st.LIST[kw.get("accumulate", 1)] if kw.get("global_sampling") else st.WINDOW
    munch = None if kw.get("n_step", 1) > 1 else (0.9, -1.0)
    off = _replays(monkeypatch, sched, **kw)
    for soft, m in (((0.5, 0.3), None), ((0.0, 0.0), None), ((0.5, 0.3), munch)):
        on = _replays(monkeypatch, sched, soft_targets=soft, **(dict(kw, munchausen=m) if m else kw))
        assert on["setup"] == off["setup"] and len(on["replays"]) == len(off["replays"])
        n_soft = 0
        for a, b in zip(on["replays"], off["replays"]):
            assert a["losses"] == b["losses"] and a["scratch"] == b["scratch"] and len(a["log"]) == len(b["log"])
            for got, was in zip(a["log"], b["log"]):
                if not was.startswith("ofx_dqn_targets"):
                    assert got == was
                    continue
                args = was[was.index("(") + 1:-1].split(", ")
                if was.startswith("ofx_dqn_targets_nstep("):
                    w, n, rows, prev, nxt, ret, disc, q, p, ya, yp = args
                    gamma = "0.9"
                else:
                    w, n, rows, prev, nxt, gamma, q, p, ya, yp = args
                    ret = disc = "None"
                alpha, clip = m if m else (0.0, 0.0)
                assert got == "ofx_dqn_targets_soft(%s)" % ", ".join(
                    [w, n, rows, prev, nxt, gamma, ret, disc, repr(soft[0]), repr(soft[1]), repr(alpha), repr(clip), q, p, ya, yp])
                n_soft += 1
        assert n_soft >= 2
    assert not any(e.startswith("ofx_dqn_targets_soft") for r in off["replays"] for e in r["log"])


def test_fingerprint_carries_the_keys_only_when_set(monkeypatch):
    off = _trainer(monkeypatch)[1].fingerprint()
    soft = _trainer(monkeypatch, soft_targets=(0.5, 0.3))[1].fingerprint()
    both = _trainer(monkeypatch, soft_targets=(0.5, 0.3), munchausen=(0.9, -1))[1].fingerprint()
    assert "soft_targets" not in off and "munchausen" not in off
    assert soft["soft_targets"] == [0.5, 0.3] and "munchausen" not in soft
    assert {k: v for k, v in soft.items() if k != "soft_targets"} == off
    assert both["munchausen"] == [0.9, -1.0] and {k: v for k, v in both.items() if k != "munchausen"} == soft


@pytest.mark.parametrize("saved,restored,key", [
    (dict(), dict(soft_targets=(0.5, 0.3)), "soft_targets"),
    (dict(soft_targets=(0.5, 0.3)), dict(), "soft_targets"),
    (dict(soft_targets=(0.5, 0.3)), dict(soft_targets=(0.5, 0.2)), "soft_targets"),
    (dict(soft_targets=(0.0, 0.0)), dict(), "soft_targets"),
    (dict(soft_targets=(0.5, 0.3)), dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0)), "munchausen"),
    (dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0)), dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -2.0)), "munchausen")])
def test_state_of_one_setting_is_refused_under_the_other(monkeypatch, saved, restored, key):
    a = _trainer(monkeypatch, **saved)[1]
    state = a.state_dict()
    batch, b = _trainer(monkeypatch, **restored)
    before = b.weights.data.copy()
    del batch.log[:]
    with pytest.raises(ValueError, match=key):
        b.load_state_dict(state)
    assert batch.log == [] and np.array_equal(b.weights.data, before)            # nothing was touched
    _trainer(monkeypatch, **saved)[1].load_state_dict(state)                     # the same setting loads
