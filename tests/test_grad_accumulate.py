"""The fit step in two halves (include/ofx.h: ofx_dqn_acc_floats, ofx_dqn_grad, ofx_dqn_apply) and
DeviceTrainer(accumulate=k) / grad_hook on top of them: the ABI, the trainer's argument checks and the fingerprint on the
CPU; on the GPU the split against the fused ofx_dqn_fit_robust bit for bit, the accumulator against numpy's float32 sum,
where the scale sits, the moving statistics and losses of a 2-chunk step, and the trainer end to end against the same
engine calls issued by hand."""
import ctypes as C

import numpy as np
import pytest
import torch    # before libofx.so is loaded (see tests/test_gpu_views.py)

SYMBOLS = ["ofx_dqn_acc_floats", "ofx_dqn_grad", "ofx_dqn_apply"]
DELTA = 0.5
TAIL, STAT, LOSS, COUNT = 256, 32, 7 * 32, 7 * 32 + 2       # OFX_ACC_TAIL, _STAT_FLOATS, _LOSS, _COUNT
WORDS = 2 * 5000                                            # uint32 words of one row's (ship, laser) bit maps


# ------------------------------------------------------------------------------------------------------ CPU
def test_split_symbols_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from ofighters_amd.engine import ArenaBatch
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s
    f, i, p = C.c_float, C.c_int32, C.c_void_p
    assert nat.SIGNATURES["ofx_dqn_acc_floats"] == (C.c_int32, [p])
    assert nat.SIGNATURES["ofx_dqn_grad"][1] == [p, p, i, p, p, p, p, p, p, f, p, i, p]
    assert nat.SIGNATURES["ofx_dqn_apply"][1] == [p, p, p, p, i, f, p, f, f, p, p]
    for m in ("dqn_acc_floats", "dqn_grad", "dqn_apply"):
        assert callable(getattr(ArenaBatch, m)), m


@pytest.mark.parametrize("value", [0, -1, 1.5, True])
def test_trainer_refuses_bad_accumulate(value):
    """before it touches the batch: batch=None would fail at replay_create"""
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match="accumulate"):
        DeviceTrainer(None, np.zeros(4, np.float32), global_sampling=True, accumulate=value)


def test_trainer_refuses_accumulate_without_global_sampling():
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match="accumulate"):
        DeviceTrainer(None, np.zeros(4, np.float32), accumulate=2)


def test_trainer_refuses_accumulate_with_reference_quirks():
    """(global_sampling is off: its own refusal of reference_quirks would come first)"""
    from ofighters_amd.trainer import DeviceTrainer
    with pytest.raises(ValueError, match="accumulate"):
        DeviceTrainer(None, np.zeros(4, np.float32), accumulate=2, reference_quirks=True)


def test_fingerprint_carries_accumulate_only_above_one(monkeypatch):
    from ofighters_amd.trainer import fingerprint_diff
    from tests.checkpoint_standin import TRAINER_KEYS, host_trainer as _trainer
    plain = _trainer(monkeypatch, global_sampling=True)
    one = _trainer(monkeypatch, global_sampling=True, accumulate=1)
    two = _trainer(monkeypatch, global_sampling=True, accumulate=2)
    assert plain.accumulate == one.accumulate == 1 and two.accumulate == 2 and two.grad_hook is None
    assert "accumulate" not in plain.fingerprint() and one.fingerprint() == plain.fingerprint()
    assert tuple(sorted(_trainer(monkeypatch).fingerprint())) == tuple(sorted(TRAINER_KEYS))
    assert two.fingerprint()["accumulate"] == 2
    assert fingerprint_diff(one.fingerprint(), two.fingerprint()) == ["accumulate"]
    two.load_state_dict(two.state_dict())
    for a, b in ((one, two), (two, one)):
        with pytest.raises(ValueError, match="accumulate"):
            b.load_state_dict(a.state_dict())


# ------------------------------------------------------------------------------------------------------ GPU
class _Off:
    """a position inside a DeviceBuffer, for the engine calls that read .ptr"""

    def __init__(self, buf, offset):
        self.ptr = buf.ptr + offset


def _targets(n):
    rs = np.random.RandomState(1)
    return rs.uniform(-1, 2, n).astype(np.float32), rs.uniform(-1, 2, n).astype(np.float32)


def _row_weights(n, seed=8):
    return np.random.RandomState(seed).uniform(0.05, 1.0, n).astype(np.float32)


class _Case:
    """One gathered minibatch (tests.fit_cases.collect_minibatch), the weights of policy_init(5), targets and row
    weights on the device; chunk(i) addresses rows [4 i, 4 i + 4) as pointer offsets."""

    def __init__(self, N, form="lean"):
        from ofighters_amd import DeviceBuffer, _native as nat
        from oracle import pyoracle
        from tests.fit_cases import collect_minibatch
        self.b, self.n, self.rows, self.bp, _ = collect_minibatch(N)
        assert self.n == 4 * N
        self.b.set_option(nat.OPT_FIT_PLAIN, int(form == "plain"))
        self.w, self.shapes = pyoracle.policy_init(5, trained_like=True)
        y, y2 = _targets(self.n)
        self.y, self.y2, self.rw = (DeviceBuffer(4 * self.n).upload(v) for v in (y, y2, _row_weights(self.n)))
        self.nf = self.w.size
        assert self.b.dqn_acc_floats() == self.nf + TAIL
        self.row_bytes = self.b.TRANSITION_DTYPE.itemsize

    def fresh(self):
        """weights, adam m, adam v"""
        from ofighters_amd import DeviceBuffer
        z = np.zeros_like(self.w)
        return [DeviceBuffer(self.w.nbytes).upload(a) for a in (self.w, z, z)]

    def acc(self, fill=None):
        from ofighters_amd import DeviceBuffer
        a = DeviceBuffer(4 * (self.nf + TAIL))
        if fill is not None:
            a.upload(np.full(self.nf + TAIL, fill, np.float32))
        return a

    def acc_host(self, acc):
        self.b.sync()
        return acc.download(np.float32, (self.nf + TAIL,))

    def chunk(self, i, rows=4):
        o = 4 * i
        return dict(n=rows, rows=self.rows.ptr + o * self.row_bytes, bp=self.bp.ptr + o * WORDS * 4, y=self.y.ptr + 4 * o,
                    y2=self.y2.ptr + 4 * o, rw=self.rw.ptr + 4 * o)

    def fused(self, ch, robust, clip=0.0, step=1):
        """ofx_dqn_fit_robust on fresh buffers -> dict of losses, norm, blobs, gradient, td"""
        from ofighters_amd import DeviceBuffer
        bufs, g, td = self.fresh(), DeviceBuffer(self.w.nbytes), DeviceBuffer(8 * ch["n"])
        l1, l2, norm = self.b.dqn_fit_robust(bufs[0], bufs[1], bufs[2], step, 1e-4, ch["n"], ch["rows"], ch["bp"], ch["y"],
                                             ch["y2"], DELTA if robust else 0.0, clip, ch["rw"] if robust else None, td.ptr, g)
        self.b.sync()
        return dict(loss=(l1, l2), norm=norm, blobs=[x.download(np.float32, self.w.shape) for x in bufs],
                    grad=g.download(np.float32, self.w.shape), td=td.download(np.float32, (ch["n"], 2)))

    def grad(self, ch, robust, acc, reset, weights, td=None, want_loss=False):
        return self.b.dqn_grad(weights, ch["n"], ch["rows"], ch["bp"], ch["y"], ch["y2"], acc, reset, DELTA if robust else 0.0,
                               ch["rw"] if robust else None, td.ptr if td else None, want_loss)

    def apply(self, acc, scale, clip, want_norm=None, step=1):
        """ofx_dqn_apply on fresh buffers"""
        bufs = self.fresh()
        l1, l2, norm = self.b.dqn_apply(bufs[0], bufs[1], bufs[2], step, 1e-4, acc, scale, clip, want_norm)
        self.b.sync()
        return dict(loss=(l1, l2), norm=norm, blobs=[x.download(np.float32, self.w.shape) for x in bufs])

    def moving(self):
        """indices of the moving means / variances in the blob"""
        idx = [np.arange(o, o + int(np.prod(shp))) for name, (o, shp) in self.shapes.items()
               if name.split(".")[1] in ("mean", "var")]
        return np.concatenate(idx)


def _same_blobs(a, b):
    for k, name in enumerate(("weights", "adam_m", "adam_v")):
        assert np.array_equal(a["blobs"][k], b["blobs"][k]), name


@pytest.mark.gpu
@pytest.mark.parametrize("robust", [False, True], ids=["no_options", "weights_huber_clip"])
@pytest.mark.parametrize("form", ["lean", "plain"])
def test_split_equals_fused_bit_for_bit(form, robust):
    """ofx_dqn_grad(reset = 1) + ofx_dqn_apply(scale = 1) against ofx_dqn_fit_robust on fresh buffers: the whole blobs,
    both losses, td and the returned norm.  With the options the clip sits at half the norm of an unclipped run."""
    from ofighters_amd import DeviceBuffer
    c = _Case(1, form)
    ch = c.chunk(0)
    clip = 0.0
    if robust:
        norm0 = c.fused(ch, True)["norm"]
        assert np.isfinite(norm0) and norm0 > 0
        clip = float(np.float32(0.5 * norm0))
    f = c.fused(ch, robust, clip)
    acc, td = c.acc(fill=np.nan), DeviceBuffer(8 * 4)
    w_d = c.fresh()[0]
    assert c.grad(ch, robust, acc, True, w_d, td) is None
    s = c.apply(acc, 1.0, clip)
    assert (f["norm"] is None) == (not robust) and s["norm"] == f["norm"]
    if robust:
        assert f["norm"] > clip                             # the clip is active
    assert s["loss"] == f["loss"] and np.isfinite(f["loss"]).all()
    assert np.array_equal(td.download(np.float32, (4, 2)), f["td"])
    assert not np.array_equal(f["blobs"][0], c.w) and np.abs(f["blobs"][1]).max() > 0
    assert not np.array_equal(f["blobs"][0][c.moving()], c.w[c.moving()])
    _same_blobs(s, f)
    c.b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lean", "plain"])
def test_grad_writes_nothing_but_the_accumulator(form):
    """... and the accumulator's layout: the fused call's grad_out, 7 stat slots with zeros behind the layer's channels,
    the two losses (returned too when asked for), a count of 1 and zeros"""
    c = _Case(1, form)
    ch = c.chunk(0)
    f = c.fused(ch, True)
    bufs = c.fresh()
    m1 = np.full(c.nf, 3, np.float32)
    bufs[1].upload(m1)
    acc = c.acc(fill=np.nan)
    loss = c.grad(ch, True, acc, True, bufs[0], want_loss=True)
    a = c.acc_host(acc)
    assert np.array_equal(bufs[0].download(np.float32, c.w.shape), c.w)
    assert np.array_equal(bufs[1].download(np.float32, c.w.shape), m1) and not bufs[2].download(np.float32, c.w.shape).any()
    assert np.array_equal(a[:c.nf], f["grad"]) and np.abs(f["grad"]).max() > 0
    assert not f["grad"][c.moving()].any()                  # untrained slots are zero
    tail = a[c.nf:]
    assert tail[COUNT] == 1.0 and (tail[LOSS], tail[LOSS + 1]) == f["loss"] == loss
    assert not tail[COUNT + 1:].any()
    for k, ch_n in enumerate((8, 8, 8, 8, 2, 4, 8)):        # trunk 0-3, head-2 0-2
        slot = tail[STAT * k:STAT * (k + 1)]
        assert np.isfinite(slot).all() and not slot[2 * ch_n:].any()
        assert (slot[1:2 * ch_n:2] > 0).all(), k            # the variances
    # the moving statistics the fused call left are 0.99 m + 0.01 stat of exactly these slots
    stat = np.concatenate([tail[STAT * k:STAT * k + 2 * n] for k, n in enumerate((8, 8, 8, 8, 2, 4, 8))])
    want = []
    for layer in ("conv1", "conv2", "conv3", "conv4", "upconv1", "upconv2", "upconv3"):
        o_m, o_v = c.shapes[layer + ".mean"][0], c.shapes[layer + ".var"][0]
        n = int(np.prod(c.shapes[layer + ".mean"][1]))
        s = stat[:2 * n]
        stat = stat[2 * n:]
        f32 = np.float32
        assert np.array_equal(f["blobs"][0][o_m:o_m + n], f32(0.99) * c.w[o_m:o_m + n] + f32(0.01) * s[0::2]), layer
        assert np.array_equal(f["blobs"][0][o_v:o_v + n], f32(0.99) * c.w[o_v:o_v + n] + f32(0.01) * s[1::2]), layer
    c.b.close()


@pytest.mark.gpu
def test_accumulation_is_the_plain_float32_sum():
    c = _Case(2)
    A, B = c.chunk(0), c.chunk(1)
    gA, gB = c.fused(A, True)["grad"], c.fused(B, True)["grad"]
    assert not np.array_equal(gA, gB)
    w_d = c.fresh()[0]
    acc = c.acc(fill=7.0)
    c.grad(A, True, acc, True, w_d)
    c.grad(B, True, acc, False, w_d)
    a = c.acc_host(acc)
    assert np.array_equal(a[:c.nf], gA + gB) and (gA + gB).dtype == np.float32
    assert a[c.nf + COUNT] == 2.0
    c.grad(B, True, acc, True, w_d)                         # reset on a dirty buffer
    a = c.acc_host(acc)
    assert np.array_equal(a[:c.nf], gB) and a[c.nf + COUNT] == 1.0
    c.b.close()


def _two_chunk_acc(c):
    w_d = c.fresh()[0]
    acc = c.acc(fill=np.nan)
    c.grad(c.chunk(0), True, acc, True, w_d)
    c.grad(c.chunk(1), True, acc, False, w_d)
    return acc


@pytest.mark.gpu
def test_where_the_scale_sits():
    """apply(acc, 0.5, clip) == apply(0.5 * acc, 1, clip) on the whole blobs: the halving on the host is exact, so the
    norm is scaled before the clip factor is formed, and Adam, the moving statistics and the losses see scale * acc"""
    from ofighters_amd import DeviceBuffer
    c = _Case(2)
    acc = _two_chunk_acc(c)
    a = c.acc_host(acc)
    free = c.apply(acc, 0.5, 0.0, want_norm=True)
    clip = float(np.float32(0.5 * free["norm"]))
    half = DeviceBuffer(a.nbytes).upload(a * np.float32(0.5))
    s, t = c.apply(acc, 0.5, clip), c.apply(half, 1.0, clip)
    assert s["norm"] == t["norm"] == free["norm"] and s["norm"] > clip
    np.testing.assert_allclose(s["norm"], 0.5 * np.sqrt((a[:c.nf].astype(np.float64) ** 2).sum()), rtol=1e-6)
    assert s["loss"] == t["loss"]
    _same_blobs(s, t)
    assert not np.array_equal(s["blobs"][1], free["blobs"][1])          # the clip acted
    c.b.close()


@pytest.mark.gpu
def test_two_chunk_step_moving_statistics_loss_and_reproducibility():
    """apply(scale = 0.5) after two chunks: 0.99 m + 0.01 (sA + sB) / 2 is the average of the two fused runs' moving
    statistics from the same start, the losses their mean; each side rounds three times in fp32 (about 8 ulp of the
    larger term), hence rtol 1e-6.  The step run twice gives the same bits."""
    c = _Case(2)
    fA, fB = c.fused(c.chunk(0), True), c.fused(c.chunk(1), True)
    s = c.apply(_two_chunk_acc(c), 0.5, 0.0)
    mv = c.moving()
    want = 0.5 * (fA["blobs"][0][mv].astype(np.float64) + fB["blobs"][0][mv].astype(np.float64))
    got = s["blobs"][0][mv].astype(np.float64)
    print("moving statistics: max relative difference %.3g" % np.max(np.abs(got - want) / np.abs(want)))
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
    assert not np.array_equal(s["blobs"][0][mv], c.w[mv])
    want_l = 0.5 * (np.array(fA["loss"], np.float64) + np.array(fB["loss"], np.float64))
    print("losses", s["loss"], want_l)
    np.testing.assert_allclose(np.array(s["loss"], np.float64), want_l, rtol=1e-6, atol=0)
    s2 = c.apply(_two_chunk_acc(c), 0.5, 0.0)
    assert s2["loss"] == s["loss"]
    _same_blobs(s2, s)
    c.b.close()


# ---- trainer ---------------------------------------------------------------------------------------------------------
T_N, T_M, T_SEED, T_FIT = 4, 4, 0x0F160077, 4


def _trainer(ticks=6, **opts):
    """A DeviceTrainer on T_N arenas (memory_size 16, fit_batch 4) after `ticks` captured collecting lock-steps"""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    from ofighters_amd.trainer import DeviceTrainer
    b = ArenaBatch(T_N, T_M)
    tr = DeviceTrainer(b, synthetic(7), learning_rate=1e-3, memory_size=16, fit_batch=T_FIT, seed=T_SEED, **opts)
    b.spawn_random(T_SEED)
    mask = np.zeros((T_N, T_M), np.uint8)
    mask[:, [0, 3]] = 1
    mask_d = DeviceBuffer(mask.nbytes).upload(mask)
    ia_d, ip_d = DeviceBuffer(4 * T_N * T_M), DeviceBuffer(8 * T_N * T_M)
    for t in range(ticks):
        b.bot_actions(["random"] * T_M, T_SEED, tick=t)
        b.policy_explore(1.0, T_SEED, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()
    return b, tr


def _step_by_hand(b, tr, k):
    """One accumulate=k replay of a fresh trainer through the engine calls: -> losses, norm, (arena, slot) fitted"""
    from ofighters_amd import DeviceBuffer, _native as nat
    fb, per = tr.fit_batch, tr.prioritized
    arena, slot, row_w, n, _ = b.replay_sample_global(tr.seed, 0, k * fb, per, tr.beta() if per else 0.0)
    assert n == k * fb
    rb = b.TRANSITION_DTYPE.itemsize
    rows, bp, bn = DeviceBuffer(n * rb), DeviceBuffer(4 * fb * WORDS), DeviceBuffer(4 * fb * WORDS)
    y, y2, td, acc = DeviceBuffer(4 * fb), DeviceBuffer(4 * fb), DeviceBuffer(8 * n), DeviceBuffer(4 * b.dqn_acc_floats())
    for i in range(k):
        o = i * fb
        rows_i = _Off(rows, o * rb)
        b.replay_gather_list_into(_Off(arena, 4 * o), _Off(slot, 4 * o), fb, rows_i, bp, bn)
        nat.check(nat.lib().ofx_dqn_targets(b.handle, tr.weights.ptr, fb, rows_i.ptr, bp.ptr, bn.ptr, 0.9, None, None,
                                             y.ptr, y2.ptr))
        b.dqn_grad(tr.weights, fb, rows_i.ptr, bp.ptr, y.ptr, y2.ptr, acc, i == 0, tr.huber_delta or 0.0,
                   row_w.ptr + 4 * o if per else None, td.ptr + 8 * o if per else None)
    l1, l2, norm = b.dqn_apply(tr.weights, tr.adam_m, tr.adam_v, 1, tr.learning_rate, acc, 1.0 / k, tr.clip_norm or 0.0)
    if per:
        b.replay_update_priorities_list(arena, slot, n, rows.ptr, td.ptr)
    b.sync()
    return (l1, l2), norm, arena.download(np.int32, (n,)), slot.download(np.int32, (n,))


def _trainer_state(b, tr):
    b.sync()
    blob = lambda buf: buf.download(np.float32, (tr.n_floats,))
    return [blob(tr.weights), blob(tr.adam_m), blob(tr.adam_v)]


def _masses(b):
    return np.concatenate([b.replay_priorities(a) for a in range(T_N)])


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [{}, dict(prioritized=True, clip_norm=1e-4)], ids=["uniform", "per_clip"])
def test_trainer_accumulate_two_is_the_engine_calls_by_hand(cfg):
    per = bool(cfg)
    b, tr = _trainer(global_sampling=True, accumulate=2, **cfg)
    w0 = tr.weights_host()
    m0 = _masses(b) if per else None
    loss = tr.replay()
    assert (tr.fit_steps, tr.draws) == (1, 1) and tr.losses == [loss] and np.isfinite(loss).all()
    assert len(tr.grad_norms) == (1 if per else 0)
    got = _trainer_state(b, tr)
    assert not np.array_equal(got[0], w0)
    b2, tr2 = _trainer(global_sampling=True, **cfg)
    loss2, norm2, arena, slot = _step_by_hand(b2, tr2, 2)
    assert loss2 == loss
    for x, y in zip(got, _trainer_state(b2, tr2)):
        assert np.array_equal(x, y)
    if per:
        assert tr.grad_norms == [norm2] and norm2 > cfg["clip_norm"]     # the clip acted on the mean gradient
        assert len(set(m0.tolist())) == 1                                # every row at the initial priority
        fitted = len(set(zip(arena.tolist(), slot.tolist())))
        m1 = _masses(b)
        assert fitted >= 2 and (m1 != m0).sum() == fitted                # all fitted rows, and only they
        assert np.array_equal(m1, _masses(b2))
    b.close(), b2.close()


@pytest.mark.gpu
def test_trainer_accumulate_one_and_hooks():
    """accumulate=1 without a hook is the trainer built without the argument; a hook on accumulate=1 goes through
    grad + apply and gives the fused step's bits; a hook that doubles the accumulator and returns 2 changes nothing
    (x 2 then x 0.5 is exact)"""
    calls = []

    def run(hook=None, **opts):
        b, tr = _trainer(global_sampling=True, huber_delta=1.0, **opts)
        names = []
        for name in ("dqn_fit_robust", "dqn_grad", "dqn_apply"):
            def wrap(fn, name=name):
                def call(*a, **kw):
                    names.append(name)
                    return fn(*a, **kw)
                return call
            setattr(b, name, wrap(getattr(b, name)))
        if hook:
            tr.grad_hook = hook
        loss = tr.replay()
        out = (loss, tr.grad_norms[:], _trainer_state(b, tr), names)
        b.close()
        return out

    def same(a, b):
        assert a[0] == b[0] and a[1] == b[1]
        for x, y in zip(a[2], b[2]):
            assert np.array_equal(x, y)

    def untouched(tr, acc):
        calls.append(acc.nbytes)
        return None

    def doubled(tr, acc):
        n = tr.batch.dqn_acc_floats()
        tr.batch.sync()
        a = acc.download(np.float32, (n,))
        assert a[n - TAIL + COUNT] == 2.0
        acc.upload(a * np.float32(2))
        return 2

    base = run()
    assert base[3] == ["dqn_fit_robust"]
    one = run(accumulate=1)
    assert one[3] == ["dqn_fit_robust"]
    same(one, base)
    hooked = run(untouched)
    assert hooked[3] == ["dqn_grad", "dqn_apply"] and len(calls) == 1
    same(hooked, base)
    two = run(accumulate=2)
    assert two[3] == ["dqn_grad", "dqn_grad", "dqn_apply"]
    assert not np.array_equal(two[2][0], base[2][0])
    same(run(doubled, accumulate=2), two)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [{}, dict(prioritized=True, clip_norm=1e-4)], ids=["uniform", "per_clip"])
def test_hook_on_the_per_arena_replay_paths(cfg):
    """without global_sampling a hook takes the step through grad + apply as well: the fused step's bits"""
    seen = []

    def run(hook):
        b, tr = _trainer(**cfg)
        tr.grad_hook = hook
        loss = tr.replay()
        assert tr.fit_steps == 1 and loss is not None
        out = (loss, tr.grad_norms[:], _trainer_state(b, tr) + ([_masses(b)] if cfg else []))
        b.close()
        return out

    base, hooked = run(None), run(lambda tr, acc: seen.append(acc) or 1)
    assert len(seen) == 1 and hooked[0] == base[0] and hooked[1] == base[1]
    for x, y in zip(hooked[2], base[2]):
        assert np.array_equal(x, y)


@pytest.mark.gpu
def test_trainer_state_round_trip():
    b, tr = _trainer(global_sampling=True, accumulate=2)
    tr.replay()
    d = tr.state_dict()
    assert d["fingerprint"]["accumulate"] == 2
    b2, tr2 = _trainer(ticks=0, global_sampling=True, accumulate=2)
    tr2.load_state_dict(d)
    assert (tr2.fit_steps, tr2.draws) == (1, 1)
    for x, y in zip(_trainer_state(b, tr), _trainer_state(b2, tr2)):
        assert np.array_equal(x, y)
    b3, tr3 = _trainer(ticks=0, global_sampling=True, accumulate=1)
    with pytest.raises(ValueError, match="accumulate"):
        tr3.load_state_dict(d)
    b.close(), b2.close(), b3.close()


# ---- errors ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_entries_refuse_bad_arguments():
    from ofighters_amd import _native as nat
    c = _Case(1)
    ch = c.chunk(0)
    bufs, acc = c.fresh(), c.acc(fill=5.0)
    L, h = nat.lib(), c.b.handle
    nan, inf = float("nan"), float("inf")

    def grad(acc_p, delta, n=4):
        return L.ofx_dqn_grad(h, bufs[0].ptr, n, ch["rows"], ch["bp"], ch["y"], ch["y2"], None, None, delta, acc_p, 1, None)

    def apply(acc_p, scale, clip, step=1):
        return L.ofx_dqn_apply(h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, step, 1e-4, acc_p, scale, clip, None, None)

    for args in ((None, 0.0), (acc.ptr, -0.5), (acc.ptr, nan), (acc.ptr, inf), (acc.ptr, 0.0, 0)):
        assert grad(*args) == nat.OFX_ERR_INVALID, args
        assert "ofx_dqn_grad" in L.ofx_last_error().decode()
    for args in ((None, 1.0, 0.0), (acc.ptr, 0.0, 0.0), (acc.ptr, -1.0, 0.0), (acc.ptr, nan, 0.0), (acc.ptr, inf, 0.0),
                 (acc.ptr, 1.0, -1.0), (acc.ptr, 1.0, nan), (acc.ptr, 1.0, inf), (acc.ptr, 1.0, 0.0, 0)):
        assert apply(*args) == nat.OFX_ERR_INVALID, args
        assert "ofx_dqn_apply" in L.ofx_last_error().decode()
    c.b.sync()
    assert np.array_equal(bufs[0].download(np.float32, c.w.shape), c.w)
    assert not bufs[1].download(np.float32, c.w.shape).any() and not bufs[2].download(np.float32, c.w.shape).any()
    assert (c.acc_host(acc) == 5.0).all()
    c.b.close()
