"""Symmetry augmentation on the GPU (include/ofx.h, "symmetry augmentation"), at 400 x 400 - the policy's only size and
the hard one, its rows being 12.5 words: ofx_obs_transform byte for byte against tests/augment_oracle.py, guard
observations around the transformed range, ofx_replay_augment on a real memory, the error list, the engine's own
rasteriser on transformed spawns, the targets and the priority write-back downstream, and a checkpointed run."""
import ctypes as C

import numpy as np
import pytest

from tests import augment_oracle as ao

pytestmark = pytest.mark.gpu

W = H = 400
WORDS = W * H // 32
SEED = 0x0F160071
SEAMS = (0, 31, 32, 367, 368, 399)                          # the word and row seams of a 12.5-word row


class _At:
    def __init__(self, buf, offset):
        self.ptr = buf.ptr + int(offset)


def _observations():
    """16 observations: the 8 elements on 50 %-dense random bits, then on single-pixel maps at the seams."""
    rng = np.random.default_rng(7)
    bits = np.zeros((16, 2, WORDS), np.uint32)
    bits[:8] = rng.integers(0, 1 << 32, (8, 2, WORDS), dtype=np.uint64).astype(np.uint32)
    for k in range(8):
        for m in range(2):
            x, y = SEAMS[(k + 3 * m) % 6], SEAMS[(2 * k + m + 1) % 6]
            p = y * W + x
            bits[8 + k, m, p >> 5] = np.uint32(1) << np.uint32(p & 31)
    vec8 = np.zeros((16, 8), np.float32)
    vec8[:, 0], vec8[:, 1], vec8[:, 4], vec8[:, 5] = rng.integers(-3, 4, 16), 1, W, H
    vec8[:, [2, 3, 6, 7]] = rng.integers(0, W, (16, 4))
    vec8[10, 6], vec8[9, 7] = W, 0                           # a ship spawned at coordinate W (under FLIP_X), one on the wall
    ptr = rng.integers(0, W, (16, 2)).astype(np.int32)
    ptr[8], ptr[9] = (0, 399), (399, 399)
    return bits, vec8, ptr, np.arange(16, dtype=np.uint8) % 8


def _oracle(ops, bits, vec8, ptr):
    return (np.stack([ao.transform_maps(int(g), b, W, H) for g, b in zip(ops, bits)]),
            np.stack([ao.transform_head(int(g), v, W, H) for g, v in zip(ops, vec8)]),
            np.stack([ao.transform_pointer(int(g), p, W, H) for g, p in zip(ops, ptr)]))


def test_obs_transform_equals_the_oracle_comes_back_and_keeps_its_neighbours():
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.engine import SYM_INVERSE
    bits, vec8, ptr, ops = _observations()
    guard = np.random.default_rng(8).integers(0, 1 << 32, (2, WORDS), dtype=np.uint64).astype(np.uint32)
    b = ArenaBatch(1, 1)
    # one guard observation before and one after the transformed range, in the same buffer
    d_bits = DeviceBuffer(18 * 2 * WORDS * 4).upload(np.concatenate([guard[None], bits, guard[None, ::-1]]))
    d_vec, d_ptr = DeviceBuffer(18 * 32).upload(np.concatenate([vec8[:1], vec8, vec8[:1]])), \
        DeviceBuffer(18 * 8).upload(np.concatenate([ptr[:1], ptr, ptr[:1]]))
    d_op = DeviceBuffer(16)
    inner = (_At(d_bits, 2 * WORDS * 4), _At(d_vec, 32), _At(d_ptr, 8))

    def read():
        b.sync()
        return (d_bits.download(np.uint32, (18, 2, WORDS)), d_vec.download(np.float32, (18, 8)), d_ptr.download(np.int32, (18, 2)))

    def guards_intact(got):
        return (got[0][0].tobytes() == guard.tobytes() and got[0][17].tobytes() == guard[::-1].tobytes() and
                got[1][0].tobytes() == got[1][17].tobytes() == vec8[0].tobytes() and
                got[2][0].tobytes() == got[2][17].tobytes() == ptr[0].tobytes())

    b.obs_transform(16, d_op.upload(ops), *inner)
    got = read()
    want = _oracle(ops, bits, vec8, ptr)
    assert guards_intact(got)
    for k in range(16):
        assert got[0][1 + k].tobytes() == want[0][k].tobytes(), "maps of observation %d (element %d)" % (k, ops[k])
    assert got[1][1:17].tobytes() == want[1].tobytes() and got[2][1:17].tobytes() == want[2].tobytes()
    assert want[1][10, 6] == -1.0 and not np.array_equal(want[0][1:8], bits[1:8])
    # the inverse elements bring the input back byte for byte
    b.obs_transform(16, d_op.upload(np.array([SYM_INVERSE[g] for g in ops], np.uint8)), *inner)
    got = read()
    assert guards_intact(got)
    assert got[0][1:17].tobytes() == bits.tobytes() and got[1][1:17].tobytes() == vec8.tobytes() and got[2][1:17].tobytes() == ptr.tobytes()
    # an op of 9 leaves its observation untouched; maps alone (no head, no pointer) work too
    odd = ops.copy()
    odd[[2, 11]] = 9, 200
    b.obs_transform(16, d_op.upload(odd), inner[0])
    got = read()
    want = _oracle(odd, bits, vec8, ptr)
    assert guards_intact(got) and got[0][1:17].tobytes() == want[0].tobytes()
    assert got[0][3].tobytes() == bits[2].tobytes() and got[0][12].tobytes() == bits[11].tobytes()
    assert got[1][1:17].tobytes() == vec8.tobytes() and got[2][1:17].tobytes() == ptr.tobytes()
    b.close()


# ---- ofx_replay_augment on a real memory -------------------------------------------------------------------------------
N, M, BATCH, DRAW = 2, 2, 8, 5


def _memory():
    """2 arenas x 2 ships, 12 captured lock-steps; arena 1 captures one ship and only from lock-step 6 on, so its memory
    holds fewer than BATCH rows and a gather pads."""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    b = ArenaBatch(N, M)
    b.replay_create(16)
    b.spawn_random(SEED)
    ia, ip, mask = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M), DeviceBuffer(N * M)
    mask.upload(np.array([[1, 1], [0, 0]], np.uint8))
    for t in range(12):
        rs = np.random.RandomState(100 + t)
        b.sync()
        ia.upload(rs.randint(0, 2, (N, M)).astype(np.int32))
        ip.upload(np.stack([rs.randint(0, W, (N, M)), rs.randint(0, H, (N, M))], -1).astype(np.int32))
        if t == 6:
            mask.upload(np.array([[1, 1], [1, 0]], np.uint8))
        b.bot_actions(["random"] * M, SEED, tick=t)
        b.replay_capture(t, mask.ptr, ia.ptr, ip.ptr)
        b.step()
    return b


def _gather(b):
    slot, _ = b.replay_sample(SEED, DRAW, BATCH)
    return b.replay_gather_device(slot, BATCH)


def _read(b, bufs):
    b.sync()
    rows, bp, bn = bufs
    return (rows.download(b.TRANSITION_DTYPE, (N * BATCH,)), bp.download(np.uint32, (N * BATCH, 2, WORDS)),
            bn.download(np.uint32, (N * BATCH, 2, WORDS)))


UNTOUCHED = ("tick_prev", "tick_next", "frame_prev", "frame_next", "ship", "iaction", "reward", "done")


def test_augment_on_a_real_memory_equals_the_oracle():
    from ofighters_amd import DeviceBuffer
    b = _memory()
    n = N * BATCH
    plain = _read(b, _gather(b))
    rows0 = plain[0]
    pads = rows0["ship"] < 0
    assert 1 <= pads.sum() <= 6 and plain[1][~pads].any(axis=(1, 2)).all() and rows0["head_prev"][~pads][:, 4].min() == W
    for mask in (0xFF, 0x55, 0xA4):
        bufs, op_out = _gather(b), DeviceBuffer(n).upload(np.full(n, 0xEE, np.uint8))
        b.replay_augment_into(SEED, DRAW, 0, n, mask, *bufs, op_out)
        got = _read(b, bufs)
        ops = op_out.download(np.uint8, (n,))
        assert np.array_equal(ops, ao.draw_ops(SEED, DRAW, 0, n, mask, ships=rows0["ship"]))
        assert (ops[pads] == 0).all() and len(set(ops[~pads].tolist())) >= 3
        want = ao.augment_rows(ops, *plain, W, H)
        assert got[0].tobytes() == want[0].tobytes()
        for k in range(n):
            assert got[1][k].tobytes() == want[1][k].tobytes() and got[2][k].tobytes() == want[2][k].tobytes(), (mask, k, ops[k])
        for f in UNTOUCHED:
            assert got[0][f].tobytes() == rows0[f].tobytes()
        assert got[0][pads].tobytes() == rows0[pads].tobytes() and not got[1][pads].any() and not got[2][pads].any()
        assert (got[0]["head_prev"][:, [0, 1, 4, 5]].tobytes() == rows0["head_prev"][:, [0, 1, 4, 5]].tobytes())
        if mask == 0xFF:
            whole = got
    # two chunks of one draw equal one call over both
    bufs, op_out = _gather(b), DeviceBuffer(n)
    rb = b.TRANSITION_DTYPE.itemsize
    for first in (0, 8):
        b.replay_augment_into(SEED, DRAW, first, 8, 0xFF, _At(bufs[0], first * rb), _At(bufs[1], first * 8 * WORDS),
                              _At(bufs[2], first * 8 * WORDS), _At(op_out, first))
    got = _read(b, bufs)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, whole))
    assert np.array_equal(op_out.download(np.uint8, (n,)), ao.draw_ops(SEED, DRAW, 0, n, 0xFF, ships=rows0["ship"]))
    # the identity alone changes nothing and reports zeros; without op_out the call works too
    bufs, op_out = _gather(b), DeviceBuffer(n).upload(np.full(n, 0xEE, np.uint8))
    b.replay_augment_into(SEED, DRAW, 0, n, 1, *bufs, op_out)
    got = _read(b, bufs)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, plain)) and not op_out.download(np.uint8, (n,)).any()
    b.replay_augment_into(SEED, DRAW, 0, n, 0xFF, *bufs)
    assert all(g.tobytes() == w.tobytes() for g, w in zip(_read(b, bufs), whole))
    b.close()


def test_invalid_arguments_are_refused_and_leave_the_buffers_untouched():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    b = _memory()
    n = N * BATCH
    bufs = _gather(b)
    plain = _read(b, bufs)
    op = DeviceBuffer(n).upload(np.full(n, 3, np.uint8))
    rows, bp, bn = (x.ptr for x in bufs)
    L, h = nat.lib(), b.handle
    aug = [(None, SEED, DRAW, 0, n, 0xFF, rows, bp, bn, None), (h, SEED, DRAW, 0, n, 0xFF, None, bp, bn, None),
           (h, SEED, DRAW, 0, n, 0xFF, rows, None, bn, None), (h, SEED, DRAW, 0, n, 0xFF, rows, bp, None, None),
           (h, SEED, DRAW, 0, 0, 0xFF, rows, bp, bn, None), (h, SEED, DRAW, 0, -1, 0xFF, rows, bp, bn, None),
           (h, SEED, DRAW, -1, n, 0xFF, rows, bp, bn, None), (h, SEED, DRAW, 2**31 - n, n, 0xFF, rows, bp, bn, None),
           (h, SEED, DRAW, 2**31 - 1, 1, 0xFF, rows, bp, bn, None),
           (h, SEED, DRAW, 0, n, 0, rows, bp, bn, None), (h, SEED, DRAW, 0, n, 0x100, rows, bp, bn, None),
           (h, SEED, DRAW, 0, n, 0x1FF, rows, bp, bn, None), (h, SEED, DRAW, 0, n, 0xFFFFFF00, rows, bp, bn, None)]
    for args in aug:
        assert L.ofx_replay_augment(*args) == nat.OFX_ERR_INVALID and L.ofx_last_error(), args
    obs = [(None, n, op.ptr, bp, None, None), (h, n, None, bp, None, None), (h, n, op.ptr, None, None, None),
           (h, 0, op.ptr, bp, None, None), (h, -4, op.ptr, bp, None, None)]
    for args in obs:
        assert L.ofx_obs_transform(*args) == nat.OFX_ERR_INVALID and L.ofx_last_error(), args
    assert all(g.tobytes() == w.tobytes() for g, w in zip(_read(b, bufs), plain))
    b.close()
    # a frame that is no square: every transposing element is refused, the flips work (rows of 6.25 words), and
    # ofx_obs_transform, which cannot see op, leaves a transposed observation untouched
    w2, h2 = 200, 64
    b = ArenaBatch(1, 1, width=w2, height=h2)
    words = w2 * h2 // 32
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 1 << 32, (8, 2, words), dtype=np.uint64).astype(np.uint32)
    rows = np.zeros(8, b.TRANSITION_DTYPE)
    rows["px"], rows["py"], rows["head_prev"][:, 6], rows["head_next"][:, 3] = 7, 9, 150, 60
    d_rows, d_p, d_n = DeviceBuffer(rows.nbytes).upload(rows), DeviceBuffer(bits.nbytes).upload(bits), DeviceBuffer(bits.nbytes).upload(bits[::-1])
    for mask in (0x02, 0xFF, 0x80, 0x57):
        with pytest.raises(OfxError) as err:
            b.replay_augment_into(SEED, 0, 0, 8, mask, d_rows, d_p, d_n)
        assert err.value.code == nat.OFX_ERR_INVALID and "width == height" in str(err.value)
    b.sync()
    assert d_p.download(np.uint32, bits.shape).tobytes() == bits.tobytes() and d_rows.download(rows.dtype, (8,)).tobytes() == rows.tobytes()
    op_out = DeviceBuffer(8)
    b.replay_augment_into(SEED, 0, 0, 8, 0x54, d_rows, d_p, d_n, op_out)
    b.sync()
    ops = op_out.download(np.uint8, (8,))
    assert np.array_equal(ops, ao.draw_ops(SEED, 0, 0, 8, 0x54)) and len(set(ops.tolist())) == 3
    want = ao.augment_rows(ops, rows, bits, bits[::-1], w2, h2)
    assert d_rows.download(rows.dtype, (8,)).tobytes() == want[0].tobytes()
    assert d_p.download(np.uint32, bits.shape).tobytes() == want[1].tobytes() and d_n.download(np.uint32, bits.shape).tobytes() == want[2].tobytes()
    d_p.upload(bits)
    each = DeviceBuffer(8).upload(np.arange(8, dtype=np.uint8))
    b.obs_transform(8, each, d_p)
    b.sync()
    got = d_p.download(np.uint32, bits.shape)
    for g in range(8):
        assert got[g].tobytes() == (bits[g] if g & 1 else ao.transform_maps(g, bits[g], w2, h2)).tobytes(), g
    b.close()
    # a frame whose two maps exceed the LDS budget
    b = ArenaBatch(1, 1, width=1024, height=512)
    big = DeviceBuffer(2 * 1024 * 512 // 8)
    row = DeviceBuffer(b.TRANSITION_DTYPE.itemsize).upload(np.zeros(1, b.TRANSITION_DTYPE))
    assert L.ofx_replay_augment(b.handle, SEED, 0, 0, 1, 0x54, row.ptr, big.ptr, big.ptr, None) == nat.OFX_ERR_INVALID
    assert b"LDS" in L.ofx_last_error()
    assert L.ofx_obs_transform(b.handle, 1, op.ptr, big.ptr, None, None) == nat.OFX_ERR_INVALID and b"LDS" in L.ofx_last_error()
    b.close()


# ---- against the engine itself -----------------------------------------------------------------------------------------
def _lsb_words(packed):
    """maps_host(MAP_BITS) rows (numpy.packbits: pixel p at bit 7 - (p & 7)) -> the stored layout (bit p & 31 of word p >> 5)."""
    return np.packbits(np.unpackbits(packed, axis=-1), axis=-1, bitorder="little").view("<u4")


def test_transforming_the_engines_observation_equals_observing_the_transformed_state():
    """Arena g of the second handle holds arena g of the first with every position under element g: its maps and heads
    must be the first handle's transformed by g, bit for bit - ships in corners and on walls, lasers at integer centres."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    ships = np.array([(0, 0), (399, 399), (8, 391), (199, 200)], np.int32)
    point = np.array([(399, 0), (17, 230), (200, 200), (0, 57)], np.int32)
    lasers = np.array([(0, 399), (398, 2), (120, 77), (201, 198), (340, 365)], np.float64)
    m = len(ships)

    def observe(elements):
        n = len(elements)
        b = ArenaBatch(n, m, laser_cap=64)
        xy = np.stack([np.stack(ao.apply_xy(g, ships[:, 0], ships[:, 1], W, H), -1) for g in elements])
        pt = np.stack([np.stack(ao.apply_xy(g, point[:, 0], point[:, 1], W, H), -1) for g in elements])
        b.spawn(np.ascontiguousarray(xy, np.int32))
        b.set_ships(x=xy[..., 0], y=xy[..., 1], px=pt[..., 0], py=pt[..., 1])
        lx, ly = np.zeros((n, 64)), np.zeros((n, 64))
        for k, g in enumerate(elements):
            lx[k, :len(lasers)], ly[k, :len(lasers)] = ao.apply_xy(g, lasers[:, 0], lasers[:, 1], W, H)
        b.sync()
        for f, a in ((nat.F_LASER_X, lx), (nat.F_LASER_Y, ly), (nat.F_N_LASERS, np.full(n, len(lasers), np.int32))):
            a = np.ascontiguousarray(a)
            nat.check(nat.lib().ofx_memcpy_h2d(nat.lib().ofx_device_ptr(b.handle, f), a.ctypes.data_as(C.c_void_p), a.nbytes))
        sm, lm = b.maps_host(nat.MAP_BITS)
        head, _ = b.observe_head()
        return b, np.stack([_lsb_words(sm), _lsb_words(lm)], 1).astype(np.uint32), head.astype(np.float32)

    b1, bits1, head1 = observe([0] * 8)
    b2, bits2, head2 = observe(list(range(8)))
    assert bits1[0, 0].any() and bits1[0, 1].any() and head1[0, :, 6].tolist() == ships[:, 0].tolist()
    ops = DeviceBuffer(8).upload(np.arange(8, dtype=np.uint8))
    d_bits = DeviceBuffer(bits1.nbytes).upload(bits1)
    for i in range(m):                                       # one observation per (arena, ship): the ship's own head
        d_bits.upload(bits1)
        d_vec = DeviceBuffer(8 * 32).upload(np.ascontiguousarray(head1[:, i]))
        b1.obs_transform(8, ops, d_bits, d_vec)
        b1.sync()
        got_bits, got_vec = d_bits.download(np.uint32, bits1.shape), d_vec.download(np.float32, (8, 8))
        for g in range(8):
            assert got_bits[g].tobytes() == bits2[g].tobytes(), g
            assert got_vec[g].tobytes() == head2[g, i].tobytes(), (g, i)
    b1.close(), b2.close()


# ---- downstream: targets and the write-back ----------------------------------------------------------------------------
def test_targets_on_an_augmented_window_keep_their_structure():
    from ofighters_amd import DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    b = _memory()
    w = synthetic(7)
    d_w = DeviceBuffer(w.nbytes).upload(w)
    slot, n_s = b.replay_sample(SEED, DRAW, BATCH)
    out = []
    for mask in (1, 0xFF):
        rows, bp, bn, n = b.replay_gather_valid(slot, n_s, BATCH, 0, N * BATCH)
        assert 8 < n < N * BATCH
        b.replay_augment_into(SEED, DRAW, 0, n, mask, rows, bp, bn)
        q_sa, p_sp, y_act, y_ptr = b.dqn_targets(d_w.ptr, n, rows.ptr, bp.ptr, bn.ptr, 0.9)
        out.append((rows.download(b.TRANSITION_DTYPE, (n,)), q_sa, p_sp, y_act, y_ptr))
        assert all(np.isfinite(v).all() for v in out[-1][1:])
    (r0, *v0), (r1, *v1) = out
    assert r0["reward"].tobytes() == r1["reward"].tobytes() and r0["done"].tobytes() == r1["done"].tobytes()
    assert not np.array_equal(r0["px"], r1["px"])
    done = r1["done"] != 0
    for v in (v0, v1):                                       # y = reward + gamma * V * (1 - done), on both
        assert np.array_equal(v[2][done], r1["reward"][done].astype(np.float32))
        assert np.array_equal(v[3][done], r1["reward"][done].astype(np.float32))
        assert (v[2][~done] != r1["reward"][~done]).all() and (v[3][~done] != r1["reward"][~done]).all()
    assert not np.array_equal(v0[0], v1[0]) and not np.array_equal(v0[3], v1[3])   # the network is not invariant: it saw other maps
    b.close()


TN, FIT, TOTAL, SPLIT = 4, 24, 26, 14


def _build(augment, is_learning=True, **kw):
    from ofighters_amd import ArenaBatch
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.lib.epsilon import Epsilon_decay
    from ofighters_amd.rollout import TrainingRollout
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(TN, M)
    eps = Epsilon_decay()
    eps.set(0.3)
    if augment != "absent":
        kw["augment"] = augment
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, epsilon=eps, batch_size=8, memory_size=16, fit_batch=FIT, **kw)
    roll = TrainingRollout(b, tr, ["random"] * M, SEED, policy_ships=(0, 1), episode_ticks=20, collecting_steps=5,
                           replay_every=3, is_learning=is_learning)
    return b, tr, roll


def test_the_write_back_finds_the_rows_of_an_augmented_replay():
    """With PER one replay moves the masses of exactly the ring rows the same replay without augment moves."""
    moved = []
    for augment in (None, "d4"):
        b, tr, roll = _build(augment, is_learning=False, prioritized=True)
        roll.run(12)                                         # fills the memories; no replay yet
        assert tr.fit_steps == 0
        before = [b.replay_priorities(a) for a in range(TN)]
        assert tr.replay() is not None and tr.fit_steps == 1
        b.sync()
        after = [b.replay_priorities(a) for a in range(TN)]
        moved.append([(x != y).tolist() for x, y in zip(before, after)])
        b.close()
    assert moved[0] == moved[1] and sum(map(sum, moved[0])) >= FIT // 2


def _state(tr):
    return tr.weights_host().tobytes(), list(tr.losses), tr.fit_steps, tr.draws


def test_a_checkpointed_run_continues_bit_for_bit_and_the_option_off_is_the_parents_run(tmp_path):
    b, tr, roll = _build("d4")
    roll.run(TOTAL)
    ref = _state(tr)
    assert tr.fit_steps >= 4 and np.isfinite(np.array(tr.losses)).all()
    b.close()
    b, tr, roll = _build("d4")
    roll.run(SPLIT)
    assert 1 <= tr.fit_steps < ref[2] - 1
    path = str(tmp_path / "ckpt")
    roll.checkpoint(path)
    b.close()
    b, tr, roll = _build("d4")
    m = roll.restore(path)
    assert m["trainer_fingerprint"]["augment"] == 0xFF
    roll.run(TOTAL - SPLIT)
    assert _state(tr) == ref
    b.close()
    for other in ("flips", None):                            # another mask is refused by the fingerprint
        b, tr, roll = _build(other)
        with pytest.raises(ValueError, match="augment"):
            roll.restore(path)
        b.close()
    # augment=None is the trainer constructed without the argument, and not the augmented run
    runs = []
    for augment in (None, "absent"):
        b, tr, roll = _build(augment)
        roll.run(TOTAL)
        assert "augment" not in tr.fingerprint()
        runs.append(_state(tr))
        b.close()
    assert runs[0] == runs[1] and runs[0][2] >= 4 and runs[0][0] != ref[0]
