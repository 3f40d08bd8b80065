"""Symmetry augmentation (include/ofx.h, "symmetry augmentation"), the part that needs no GPU: the two entry points are
exported, declared and bound; the oracle's group tables are a group's; the transformation commutes with the CPU oracle's
rasteriser; and DeviceTrainer(augment=...) on the recording stand-ins of tests/replay_standin.py - what is refused
before any device call, the fingerprint, and where the one new call stands in a replay."""
import ctypes as C
import re

import numpy as np
import pytest

from ofighters_amd import _native as nat
from ofighters_amd import engine
from oracle import pyoracle
from tests import augment_oracle as ao
from tests import replay_standin as st
from tests.abi_header import ROOT, header_symbols

W = H = 400


# ---- symbols -----------------------------------------------------------------------------------------------------------
def test_both_entry_points_are_exported_declared_and_bound():
    L = C.CDLL(nat.LIB_PATH)
    syms = header_symbols()
    for name, n_args in (("ofx_obs_transform", 6), ("ofx_replay_augment", 10)):
        assert hasattr(L, name) and name in syms
        res, args = nat.SIGNATURES[name]
        assert res is C.c_int and len(args) == n_args
        src = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/ofx.h").read(), flags=re.S)
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, src).group(1)
        assert len(decl.split(",")) == n_args
    assert nat.SIGNATURES["ofx_replay_augment"][1][1:6] == [C.c_uint64, C.c_uint32, C.c_int32, C.c_int32, C.c_uint32]
    assert (engine.OFX_SYM_TRANSPOSE, engine.OFX_SYM_FLIP_X, engine.OFX_SYM_FLIP_Y) == (1, 2, 4)
    hdr = open(ROOT + "/include/ofx.h").read()
    for name, val in (("OFX_SYM_TRANSPOSE", 1), ("OFX_SYM_FLIP_X", 2), ("OFX_SYM_FLIP_Y", 4)):
        assert re.search(r"#define %s\s+%d\b" % (name, val), hdr)


# ---- tables ------------------------------------------------------------------------------------------------------------
def _random_obs(seed):
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 32, (2, W * H // 32), dtype=np.uint64).astype(np.uint32)
    vec8 = np.array([3, 1, rng.integers(0, W), rng.integers(0, H), W, H, rng.integers(0, W), rng.integers(0, H)], np.float32)
    ptr = rng.integers(0, W, 2).astype(np.int32)
    return bits, vec8, ptr


def _apply(g, obs):
    bits, vec8, ptr = obs
    return ao.transform_maps(g, bits, W, H), ao.transform_head(g, vec8, W, H), ao.transform_pointer(g, ptr, W, H)


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_engine_tables_are_the_oracles():
    assert list(engine.SYM_INVERSE) == ao.INVERSE == [0, 1, 2, 5, 4, 3, 6, 7]
    assert [list(r) for r in engine.SYM_COMPOSE] == ao.COMPOSE
    hdr = open(ROOT + "/include/ofx.h").read()                     # the contract carries both tables
    assert "{0, 1, 2, 5, 4, 3, 6, 7}" in hdr
    for row in ao.COMPOSE:
        assert "{%s}" % ", ".join(map(str, row)) in hdr


def test_every_element_composed_with_its_inverse_is_the_identity():
    obs = _random_obs(1)
    for g in range(8):
        there = _apply(g, obs)
        assert (g == 0) == _same(there, obs)
        assert _same(_apply(engine.SYM_INVERSE[g], there), obs)
        assert engine.SYM_COMPOSE[g][engine.SYM_INVERSE[g]] == 0 == engine.SYM_COMPOSE[engine.SYM_INVERSE[g]][g]
    assert _same(_apply(9, obs), obs)                               # not an element: untouched


def test_compose_agrees_with_applying_two_elements_in_turn():
    obs = _random_obs(2)
    once = [_apply(g, obs) for g in range(8)]
    for a in range(8):
        for b in range(8):
            assert _same(_apply(b, once[a]), once[engine.SYM_COMPOSE[a][b]]), (a, b)


def test_a_map_pixel_moves_where_the_position_formula_says():
    for (x, y) in ((0, 0), (31, 32), (399, 0), (367, 368), (5, 399)):
        img = np.zeros((H, W), np.uint8)
        img[y, x] = 1
        bits = np.stack([ao.pack_map(img), ao.pack_map(img)])
        for g in range(8):
            out = ao.unpack_map(ao.transform_maps(g, bits, W, H)[0], W, H)
            x2, y2 = ao.apply_xy(g, x, y, W, H)
            assert out.sum() == 1 and out[y2, x2] == 1
            assert ao.transform_pointer(g, (x, y), W, H).tolist() == [x2, y2]
            v = ao.transform_head(g, np.array([7, 1, x, y, W, H, y, x], np.float32), W, H)
            assert v.tolist() == [7, 1, x2, y2, W, H] + list(ao.apply_xy(g, y, x, W, H))
    assert ao.transform_head(2, np.array([0, 1, 0, 0, W, H, W, 3], np.float32), W, H)[6] == -1.0   # a ship spawned at W


# ---- equivariance with the rasteriser ----------------------------------------------------------------------------------
SHIPS = [(0, 0), (399, 399), (8, 391), (199, 200), (57, 123), (300, 41), (250, 250)]
LASERS = [(0, 399), (399, 1), (2, 2), (120, 77), (201, 198), (340, 365)]


def _raster(ships, lasers):
    a = pyoracle.Arena(n_ships=len(ships))
    a.spawn(np.zeros((len(ships), 2), np.int32))
    for i, (x, y) in enumerate(ships):
        a.set_ship(i, x, y, 0, 0)
    sm = a.rasterise()[0]
    lm = np.zeros((H, W), np.uint8)
    for x, y in lasers:
        lm |= pyoracle.disk(y, x, a.cfg.laser_radius)
    return sm, lm


def test_the_disc_is_symmetric_about_an_integer_centre():
    """What the contract assumes: disk() around an integer centre is invariant under all eight elements about it."""
    for radius in (8, 2):
        d = pyoracle.disk(20, 20, radius, 41, 41)
        assert d.sum() > 4
        for g in range(8):
            assert np.array_equal(ao.transform_image(g, d), d)


def test_transforming_the_map_equals_rasterising_the_transformed_centres():
    sm, lm = _raster(SHIPS, LASERS)
    assert sm.sum() > 800 and lm.sum() > 40
    bits = np.stack([ao.pack_map(sm), ao.pack_map(lm)])
    for g in range(8):
        sm2, lm2 = _raster([ao.apply_xy(g, x, y, W, H) for x, y in SHIPS], [ao.apply_xy(g, x, y, W, H) for x, y in LASERS])
        got = ao.transform_maps(g, bits, W, H)
        assert got[0].tobytes() == ao.pack_map(sm2).tobytes(), g
        assert got[1].tobytes() == ao.pack_map(lm2).tobytes(), g


# ---- the draw ----------------------------------------------------------------------------------------------------------
def test_draws_stay_in_the_mask_split_like_one_call_and_skip_padding_rows():
    for mask in (0xFF, 0x55, 0x24, 0x01, 0x80):
        ops = ao.draw_ops(11, 3, 0, 64, mask)
        assert all(mask >> int(g) & 1 for g in ops)
        assert np.array_equal(np.concatenate([ao.draw_ops(11, 3, 0, 24, mask), ao.draw_ops(11, 3, 24, 40, mask)]), ops)
    ops = ao.draw_ops(11, 3, 0, 64, 0xFF)
    assert len(set(ops.tolist())) == 8
    assert not np.array_equal(ops, ao.draw_ops(11, 4, 0, 64, 0xFF)) and not np.array_equal(ops, ao.draw_ops(12, 3, 0, 64, 0xFF))
    assert not np.array_equal(ops, ao.draw_ops(11, 3, 0, 64, 0xFF, arena_base=64))
    ships = np.arange(64) % 3 - 1                                   # every third row is a padding row
    padded = ao.draw_ops(11, 3, 0, 64, 0xFE, ships=ships)
    assert (padded[ships < 0] == 0).all() and (padded[ships >= 0] > 0).all()
    r = pyoracle.philox(0, 5, 3, ao.STREAM_AUGMENT, 11)
    assert ao.draw_ops(11, 3, 5, 1, 0xA4)[0] == [2, 5, 7][(int(r[0]) * 3) >> 32]


# ---- DeviceTrainer(augment=) -------------------------------------------------------------------------------------------
class AugmentRecordingBatch(st.RecordingBatch):
    """The recording stand-in with the one call the option adds, logged like every other."""

    def replay_augment_into(self, seed, draw, first, n, op_mask, rows, bits_prev, bits_next, op_out=None):
        self._log("replay_augment_into", (seed, draw, first, n, op_mask, rows, bits_prev, bits_next, op_out))

    def dqn_targets_soft_into(self, w, n, rows_p, prev_p, next_p, gamma, y_act_p, y_ptr_p, tau_act, tau_ptr, m_alpha=0.0,
                              m_clip=0.0, ret_p=None, disc_p=None, q_sa_p=None, p_sp_p=None):
        self._log("ofx_dqn_targets_soft", (w, n, rows_p, prev_p, next_p, float(gamma), ret_p, disc_p, tau_act, tau_ptr, m_alpha,
                                            m_clip, q_sa_p, p_sp_p, y_act_p, y_ptr_p))


def _trainer(monkeypatch, **kw):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch = AugmentRecordingBatch()
    t = tr.DeviceTrainer(batch, np.arange(st.N_FLOATS, dtype=np.float32), **dict(st.COMMON, **kw))
    batch.trainer = t
    return batch, t


def test_accepted_values_become_masks(monkeypatch):
    for arg, want in ((None, None), ("flips", 0x55), ("d4", 0xFF), (1, 1), (255, 255), (0x24, 0x24), (np.int32(6), 6)):
        t = _trainer(monkeypatch, augment=arg)[1]
        assert t.augment == want and (want is None or type(t.augment) is int)
    assert _trainer(monkeypatch)[1].augment is None


BAD = [0, 256, -1, True, False, "D4", "rot", "", 1.0, 0.5, (1, 2), [0x55], np.bool_(True), b"d4", float("nan")]


@pytest.mark.parametrize("bad", BAD, ids=[repr(b) for b in BAD])
def test_bad_values_are_refused_before_any_device_call(monkeypatch, bad):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch, made = AugmentRecordingBatch(), st.HostBuffer.count
    with pytest.raises(ValueError, match="augment"):
        tr.DeviceTrainer(batch, np.zeros(4, np.float32), augment=bad)
    assert batch.log == [] and st.HostBuffer.count == made


@pytest.mark.parametrize("value", ["flips", "d4", 3])
def test_refused_with_reference_quirks(monkeypatch, value):
    import ofighters_amd.trainer as tr
    monkeypatch.setattr(tr, "DeviceBuffer", st.HostBuffer)
    batch, made = AugmentRecordingBatch(), st.HostBuffer.count
    with pytest.raises(ValueError, match="augment"):
        tr.DeviceTrainer(batch, np.zeros(4, np.float32), augment=value, reference_quirks=True)
    assert batch.log == [] and st.HostBuffer.count == made


def test_fingerprint_carries_the_mask_only_when_set(monkeypatch):
    off = _trainer(monkeypatch)[1].fingerprint()
    on = _trainer(monkeypatch, augment="d4")[1].fingerprint()
    assert "augment" not in off and on["augment"] == 0xFF
    assert {k: v for k, v in on.items() if k != "augment"} == off
    assert _trainer(monkeypatch, augment="flips")[1].fingerprint()["augment"] == 0x55
    assert _trainer(monkeypatch, augment=1)[1].fingerprint()["augment"] == 1      # the identity alone is still "set"


@pytest.mark.parametrize("saved,restored", [(dict(), dict(augment="d4")), (dict(augment="d4"), dict()),
                                            (dict(augment="d4"), dict(augment="flips"))])
def test_state_of_one_mask_is_refused_under_another(monkeypatch, saved, restored):
    state = _trainer(monkeypatch, **saved)[1].state_dict()
    batch, b = _trainer(monkeypatch, **restored)
    before = b.weights.data.copy()
    del batch.log[:]
    with pytest.raises(ValueError, match="augment"):
        b.load_state_dict(state)
    assert batch.log == [] and np.array_equal(b.weights.data, before)
    _trainer(monkeypatch, **saved)[1].load_state_dict(state)


def _replays(monkeypatch, sched, **kw):
    batch, t = _trainer(monkeypatch, **kw)
    out = []
    for step in sched:
        del batch.log[:]
        batch.step = step
        t.replay()
        out.append({"log": list(batch.log), "losses": list(t.losses), "draws": t.draws,
                    "scratch": {k: b.nbytes for k, b in sorted(t._buf.items())}})
    return out


def _args(entry):
    return entry[entry.index("(") + 1:-1].split(", ")


GATHERS = ("replay_gather_valid_into(", "replay_gather_nstep_into(", "replay_gather_list_into(")
TARGETS = ("ofx_dqn_targets", "dqn_targets_double_into(")
SAMPLERS = ("replay_sample(", "replay_sample_prioritized(", "replay_sample_global(")
CALL_LOG = [dict(), dict(prioritized=True), dict(n_step=3), dict(global_sampling=True),
            dict(global_sampling=True, accumulate=3), dict(global_sampling=True, accumulate=3, n_step=3, prioritized=True),
            dict(soft_targets=(0.5, 0.3), munchausen=(0.9, -1.0)), dict(double_dqn=True, target_sync=2, huber_delta=1.0)]


@pytest.mark.parametrize("kw", CALL_LOG, ids=[repr(k) for k in CALL_LOG])
def test_one_augment_call_per_chunk_between_its_gather_and_its_targets(monkeypatch, kw):
    acc = kw.get("accumulate", 1)
    sched = st.WINDOW if not kw.get("global_sampling") else \
        [dict(drawn=21), dict(drawn=24), dict(drawn=5)] if acc == 3 else st.LIST[acc]
    off = _replays(monkeypatch, sched, **kw)
    on = _replays(monkeypatch, sched, augment="d4", **kw)
    assert not any(e.startswith("replay_augment_into") for r in off for e in r["log"])      # augment=None: no such call
    row_bytes, fb, n_calls, multi = engine.ArenaBatch.TRANSITION_DTYPE.itemsize, st.COMMON["fit_batch"], 0, False
    for a, b in zip(on, off):
        assert a["losses"] == b["losses"] and a["scratch"] == b["scratch"] and a["draws"] == b["draws"]
        log = a["log"]
        assert [e for e in log if not e.startswith("replay_augment_into")] == b["log"]       # nothing else moved
        sampled = [_args(e)[1] for e in log if e.startswith(SAMPLERS)]
        assert len(sampled) == 1 and int(sampled[0]) == a["draws"] - 1
        gathers = [i for i, e in enumerate(log) if e.startswith(GATHERS)]
        assert len(gathers) == sum(e.startswith("replay_augment_into") for e in log) >= 1
        multi |= len(gathers) > 1
        for chunk, i in enumerate(gathers):
            g = _args(log[i])
            t = next(k for k in range(i, len(log)) if log[k].startswith(TARGETS))               # this chunk's targets
            assert log[t - 1].startswith("replay_augment_into(")
            assert all(e.startswith("replay_window_weights_into(") for e in log[i + 1:t - 1])   # part of a PER window's gather
            m = int(g[2]) if log[i].startswith("replay_gather_list_into(") else int(g[4])
            assert m == (fb if len(gathers) > 1 else m)
            o = chunk * m
            assert _args(log[t - 1]) == [str(st.COMMON["seed"]), sampled[0], str(o), str(m), "255", "rows+%d" % (o * row_bytes),
                                         "bits_prev+0", "bits_next+0", "None"]
            n_calls += 1
    assert n_calls >= 3 and multi == (acc > 1)
