"""The forward on stored observations (ofx_policy_forward_obs) and the TD targets built on it (ofx_dqn_targets,
ofx_dqn_targets_nstep) at the sizes training uses: from 4 * n_cus observations (1024 on an MI355X) the trunk runs as the
streaming kernels (k_trunk12<0, true>, k_conv3_stream<0>) with the sparse form forced on, the two maps of an observation
interleaved (bits_stride = 2 * words) and one head per image.

Two yardsticks.
  EXACT        include/ofx.h: OFX_OPT_TRUNK_FUSE is 'bit-identical either way', the sparse form is 'BIT-IDENTICAL to the
               dense form', and an observation's result does not depend on the batch it sits in.  So every row of a large
               batch is compared (np.array_equal, no row excluded) with the same call under OFX_OPT_TRUNK_FUSE = 2 - the
               two-kernel dense trunk: no streaming, no sparse skipping, no persistent loop - and a subset with the
               one-observation call under OFX_OPT_TRUNK_FUSE = 2.
  INDEPENDENT  the float64 graph (tests/policy_ref64.py) on a sample of the rows, with the tolerances of
               tests/test_gpu_policy_fp64.py (4 x the largest error measured on the chip).

That the path under test ran is read from ofx_policy_trunk_stats (OFX_OPT_TRUNK_SPARSE = 1 around the calls: the results
are unchanged, the counters become live): n * 20 * 63 M-tiles for n images through the streaming trunk, zeros for the
two-kernel form.  An auto-mode case that finds zeros FAILS: the streaming path was not taken.

Wall time on an MI355X, both files in one run: this file 5.8 s (23 tests; the 64 float64 forwards of the minibatch sample
are 3.5 s of it), tests/test_gpu_policy_fp64.py 13.4 s."""
import numpy as np
import pytest

from tests import obs_batches as OB
from tests.frame_cases import CASES as FRAME_CASES, frame_weights, where
from tests.policy_fp64_cases import TOL_ACT, TOL_HEAT, report as _report

pytestmark = pytest.mark.gpu

N, M, CAP, TICKS, EPISODE, SEED = 16, 8, 192, 90, 30, 0x0F160011
POLICY_SHIPS = (0, 3)
GAMMA, NSTEP, ROWS = 0.9, 3, 1500
TILES_PER_IMAGE = 20 * 63            # 20 steps of 20 rows, 63 M-tiles of 16 pixels each (test_trunk_sparse_is_bit_identical)
KEYS = ("act", "iaction", "ipointer", "ptr_max", "ptr_probe")
ROW_BYTES, VEC_BYTES, PROBE_BYTES = 2 * OB.WORDS * 4, 32, 8

_S = {}


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    for k in ("b", "sb"):
        if _S.get(k) is not None:
            _S[k].close()
    _S.clear()


# ---------------------------------------------------------------------------------------------- the path that ran
def _check_path(st, images, path, what):
    run, total = st[0], st[1]
    if path == "stream":
        assert total != 0, "%s: no M-tile was counted - the streaming trunk was NOT taken" % what
        assert total == images * TILES_PER_IMAGE and 0 < run <= total, (what, st, images)
    else:
        assert tuple(st) == (0, 0, 0, 0), "%s: the two-kernel form was expected, the streaming trunk counted %r" % (what, st)


class _Options:
    """OFX_OPT_TRUNK_FUSE = fuse and OFX_OPT_TRUNK_SPARSE = 1 around a block; .stats after it."""

    def __init__(self, b, fuse):
        self.b, self.fuse = b, fuse

    def __enter__(self):
        from ofighters_amd import _native as nat
        self.b.set_option(nat.OPT_TRUNK_FUSE, self.fuse)
        self.b.set_option(nat.OPT_TRUNK_SPARSE, 1)
        self.b.policy_trunk_stats()
        return self

    def __exit__(self, *exc):
        from ofighters_amd import _native as nat
        try:
            self.stats = self.b.policy_trunk_stats()
        finally:
            self.b.set_option(nat.OPT_TRUNK_FUSE, 0)
            self.b.set_option(nat.OPT_TRUNK_SPARSE, 0)
        return False


def _forward(b, w_d, n, bits_ptr, vec_ptr, probe_ptr, fuse, path, what):
    with _Options(b, fuse) as o:
        out = b.policy_forward_obs(w_d.ptr, n, bits_ptr, vec_ptr, probe_ptr)
    print("%-44s n %4d fuse %d: M-tiles run %d of %d, table passes run %d of %d" % ((what, n, fuse) + tuple(o.stats)))
    _check_path(o.stats, n, path, what)
    return out, o.stats


def _assert_same(got, want, what, rows=None):
    for k in KEYS:
        if k in want or k in got:
            a, r = got[k], (want[k] if rows is None else want[k][rows])
            if not np.array_equal(a, r):
                bad = np.flatnonzero((a != r).reshape(len(a), -1).any(axis=1))
                raise AssertionError("%s: %s differs in %d of %d rows, first %s (image index mod 256: %s): %r != %r" % (
                    what, k, len(bad), len(a), bad[:12], bad[:12] % 256, a[bad[0]], r[bad[0]]))


# ---------------------------------------------------------------------------------------------- a real minibatch
def _play(b, mask_d, ia_d, ip_d, ticks=TICKS):
    """Lock-steps of turret and random bots around the capturing ships (device exploration, collecting phase), episodes
    of EPISODE lock-steps: ships die and respawn, the capture clock runs on."""
    beh = ["turret" if i % 2 else "random" for i in range(M)]
    for t in range(ticks):
        if t and t % EPISODE == 0:
            b.restart_random(SEED)
        b.bot_actions(beh, SEED, tick=t)
        b.policy_explore(1.0, SEED, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()


def _capture_buffers(n_arenas):
    from ofighters_amd import DeviceBuffer
    mask = np.zeros((n_arenas, M), np.uint8)
    mask[:, POLICY_SHIPS] = 1
    return DeviceBuffer(mask.nbytes).upload(mask), DeviceBuffer(4 * n_arenas * M), DeviceBuffer(8 * n_arenas * M)


def _side(rows, which):
    """Device heads (and, for `state`, the probes) of gathered rows, as ofx_dqn_targets unpacks them."""
    from ofighters_amd import DeviceBuffer
    vec = np.ascontiguousarray(rows["head_" + which], np.float32)
    out = dict(vec=vec, vec_d=DeviceBuffer(vec.nbytes).upload(vec), probe=None, probe_d=None)
    if which == "prev":
        out["probe"] = np.ascontiguousarray(np.stack([rows["px"], rows["py"]], 1), np.int32)
        out["probe_d"] = DeviceBuffer(out["probe"].nbytes).upload(out["probe"])
    return out


def _minibatch():
    """Every eligible row of every arena, sampled (batch = capacity) and packed: the first ROWS of them."""
    if "mb" in _S:
        return _S["mb"]
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from oracle import pyoracle
    b = _S["b"] = ArenaBatch(N, M)
    b.replay_create(CAP, 0)
    b.spawn_random(SEED)
    _play(b, *_capture_buffers(N))
    slot, n_s = b.replay_sample(7, 0, CAP)
    b.sync()
    n_h = n_s.download(np.int32, (N,))
    total = int(n_h.sum())
    assert total >= ROWS and (n_h < CAP).all(), (total, n_h)          # every arena leaves pads in the padded form
    rows_d, bp_d, bn_d, got = b.replay_gather_valid(slot, n_s, CAP, 0, ROWS)
    assert got == ROWS
    rows = rows_d.download(b.TRANSITION_DTYPE, (ROWS,))
    assert (rows["ship"] >= 0).all()
    assert (rows["px"] >= 0).all() and (rows["px"] < 400).all() and (rows["py"] >= 0).all() and (rows["py"] < 400).all()
    n_done, n_reward = int((rows["done"] != 0).sum()), int((rows["reward"] != 0).sum())
    print("minibatch: %d sampled rows in %d arenas, window of %d: done %d, rewarded %d" % (total, N, ROWS, n_done, n_reward))
    assert n_done >= 8 and n_reward >= 8, (n_done, n_reward)
    w, _ = pyoracle.policy_init(6, trained_like=True)
    mb = dict(b=b, slot=slot, n_s=n_s, n_h=n_h, total=total, rows=rows, rows_d=rows_d, w=w,
              w_d=DeviceBuffer(w.nbytes).upload(w), fwd={},
              next=dict(bits_d=bn_d, **_side(rows, "next")), prev=dict(bits_d=bp_d, **_side(rows, "prev")))
    _S["mb"] = mb
    return mb


def _mb_forward(mb, side, n, fuse, path):
    """forward_obs on the first n rows of the window (cached per (side, n, fuse))."""
    key = (side, n, fuse)
    if key not in mb["fwd"]:
        s = mb[side]
        mb["fwd"][key] = _forward(mb["b"], mb["w_d"], n, s["bits_d"].ptr, s["vec_d"].ptr, s["probe_d"].ptr if s["probe_d"] else None,
                                  fuse, path, "minibatch %s" % side)[0]
    return mb["fwd"][key]


def _sample_rows(mb, count=32):
    """Rows of the window for the float64 comparison: done rows, rewarded rows, the ends, random ones."""
    rows = mb["rows"]
    rs = np.random.RandomState(17)
    pick = set(map(int, np.flatnonzero(rows["done"] != 0)[:8])) | {0, ROWS - 1}
    pick |= set(map(int, np.flatnonzero((rows["reward"] != 0) & (rows["done"] == 0))[:8]))
    rest = [int(i) for i in rs.permutation(ROWS) if int(i) not in pick]
    pick = np.array(sorted(pick) + rest[:count - len(pick)])
    pick.sort()
    assert len(pick) == count == len(set(pick))
    assert (rows["done"][pick] != 0).sum() >= 8 and (rows["reward"][pick] != 0).sum() >= 8
    return pick


def _f64(bits_row, vec8, w, legacy=False):
    import torch
    from tests import policy_ref64 as R
    torch.set_num_threads(16)
    m = OB.unpack_maps(bits_row[None])[0]
    a, h = R.forward(m[0], m[1], np.asarray(vec8, np.float32)[None], w, legacy_bilinear=legacy)
    return a[0], h[0]


def _mb_fp64(mb):
    """float64 forwards of the sampled rows, once: {side: {row: (act64, heat64)}}."""
    if "f64" not in mb:
        pick = _sample_rows(mb)
        out = dict(pick=pick, prev={}, next={})
        for side in ("prev", "next"):
            for i in pick:
                bits = mb[side]["bits_d"].download(np.uint32, (2, OB.WORDS), offset=int(i) * ROW_BYTES)
                out[side][int(i)] = _f64(bits, mb[side]["vec"][i], mb["w"])
        mb["f64"] = out
    return mb["f64"]


class _Worst:
    """The float64 comparison of tests/test_gpu_policy_fp64.py on the outputs of forward_obs: figures first, then the verdict."""

    def __init__(self):
        self.act = self.ptr_max = self.ptr_probe = 0.0
        self.n = self.skipped = self.argmax_same = 0
        self.bad = []

    def add(self, out, i, a64, h64, probe, tag):
        sa, hs = max(1.0, float(np.abs(a64).max())), float(np.abs(h64).max())
        ea = float(np.abs(out["act"][i].astype(np.float64) - a64).max()) / sa
        em = abs(float(out["ptr_max"][i]) - float(h64.max())) / hs
        self.act, self.ptr_max, self.n = max(self.act, ea), max(self.ptr_max, em), self.n + 1
        if ea > TOL_ACT:
            self.bad.append((tag, "act", ea))
        if em > TOL_HEAT:
            self.bad.append((tag, "ptr_max", em))
        if probe is not None:
            ep = abs(float(out["ptr_probe"][i]) - float(h64[probe[1], probe[0]])) / hs
            self.ptr_probe = max(self.ptr_probe, ep)
            if ep > TOL_HEAT:
                self.bad.append((tag, "ptr_probe", ep))
        gx, gy = (int(v) for v in out["ipointer"][i])
        self.argmax_same += int(gy * 400 + gx == int(np.argmax(h64)))
        if not h64[gy, gx] >= h64.max() - 2 * TOL_HEAT * hs:
            self.bad.append((tag, "ipointer", (gx, gy), float(h64[gy, gx]), float(h64.max())))
        if abs(float(a64[0] - a64[1])) > 2 * TOL_ACT * sa:
            if int(out["iaction"][i]) != int(np.argmax(a64)):
                self.bad.append((tag, "iaction", int(out["iaction"][i])))
        else:
            self.skipped += 1

    def record(self):
        return dict(act=self.act, ptr_max=self.ptr_max, ptr_probe=self.ptr_probe, argmax_same=self.argmax_same,
                    iaction_skipped=self.skipped, forwards=self.n)

    def verdict(self, tag):
        _report(tag, self.record())
        assert not self.bad, self.bad
        assert 8 * self.skipped <= self.n, "iaction was near a tie in %d of %d forwards: take another policy_init seed" % (self.skipped, self.n)


# ---------------------------------------------------------------------------------------------- 1. real minibatches
@pytest.mark.parametrize("n,fuse,path", [(1500, 0, "stream"), (1024, 0, "stream"), (1023, 0, "split"), (257, 1, "stream"),
                                         (3, 1, "stream")])
def test_minibatch_forward_equals_the_two_kernel_form(n, fuse, path):
    """1500 rows (not a multiple of the 256-block grid: blocks walk 5 or 6 images), 1024 (the threshold itself), 1023
    (one below: the two-kernel form by itself, and equal to the first 1023 rows of the 1500-row streaming result - the
    threshold pinned from both sides), 257 and 3 rows forced through the streaming trunk: every row, both observations of
    the transitions (`state` with the probe at the chosen pointer), equal to the call under OFX_OPT_TRUNK_FUSE = 2."""
    mb = _minibatch()
    for side in ("next", "prev"):
        got = _mb_forward(mb, side, n, fuse, path)
        assert ("ptr_probe" in got) == (side == "prev")
        _assert_same(got, _mb_forward(mb, side, n, 2, "split"), "%s, %d rows, fuse %d vs 2" % (side, n, fuse))
        # ... and the observation's result does not depend on the batch: the prefix of the 1500-row calls
        _assert_same(got, _mb_forward(mb, side, ROWS, 0, "stream"), "%s, %d rows vs the 1500-row call" % (side, n), slice(0, n))
        _assert_same(got, _mb_forward(mb, side, ROWS, 2, "split"), "%s, %d rows vs the 1500-row call, fuse 2" % (side, n), slice(0, n))


def test_minibatch_rows_equal_their_one_observation_calls():
    """A subset of the 1500 rows - done rows, rewarded rows, the rows around the grid's multiples - against n_obs = 1."""
    mb = _minibatch()
    rows = mb["rows"]
    pick = sorted(set([0, 1, 255, 256, 257, 511, 512, 1023, 1024, 1279, 1280, ROWS - 1]
                      + list(np.flatnonzero(rows["done"] != 0)[:3]) + list(np.flatnonzero(rows["reward"] != 0)[:3])))
    for side in ("next", "prev"):
        s, big = mb[side], _mb_forward(mb, side, ROWS, 0, "stream")
        for i in pick:
            i = int(i)
            one, _ = _forward(mb["b"], mb["w_d"], 1, s["bits_d"].ptr + i * ROW_BYTES, s["vec_d"].ptr + i * VEC_BYTES,
                              s["probe_d"].ptr + i * PROBE_BYTES if s["probe_d"] else None, 2, "split", "row %d alone" % i)
            _assert_same(one, big, "%s row %d alone vs in the 1500-row call" % (side, i), slice(i, i + 1))


def test_minibatch_forward_against_fp64():
    """32 rows of the 1500-row streaming call, both observations (64 forwards), against the float64 graph."""
    mb = _minibatch()
    f64 = _mb_fp64(mb)
    worst = _Worst()
    for side in ("prev", "next"):
        out = _mb_forward(mb, side, ROWS, 0, "stream")
        for i in f64["pick"]:
            a64, h64 = f64[side][int(i)]
            worst.add(out, int(i), a64, h64, mb[side]["probe"][i] if side == "prev" else None, "%s row %d" % (side, i))
    worst.verdict("forward_obs_1500")


# ---------------------------------------------------------------------------------------------- 2. the targets
def _targets(mb, kind, n, rows_d, bp_d, bn_d, extra, current, fuse, path, what):
    b = mb["b"]
    with _Options(b, fuse) as o:
        if kind == "one_step":
            out = b.dqn_targets(mb["w_d"].ptr, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, GAMMA, current=current)
        else:
            out = b.dqn_targets_nstep(mb["w_d"].ptr, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, extra[0].ptr, extra[1].ptr, current=current)
    print("%-44s n %4d fuse %d current %d: M-tiles run %d of %d" % (what, n, fuse, current, o.stats[0], o.stats[1]))
    _check_path(o.stats, n * (2 if current else 1), path, what)
    return out


def _nstep_window(mb):
    if "nstep" not in mb:
        from ofighters_amd import DeviceBuffer
        b = mb["b"]
        rows_d = DeviceBuffer(ROWS * b.TRANSITION_DTYPE.itemsize)
        bp_d, bn_d = DeviceBuffer(ROWS * ROW_BYTES), DeviceBuffer(ROWS * ROW_BYTES)
        ret_d, disc_d = DeviceBuffer(4 * ROWS), DeviceBuffer(4 * ROWS)
        got = b.replay_gather_nstep_into(mb["slot"], mb["n_s"], CAP, 0, ROWS, NSTEP, GAMMA, rows_d, bp_d, bn_d, ret_d, disc_d)
        assert got == ROWS
        rows = rows_d.download(b.TRANSITION_DTYPE, (ROWS,))
        ret, disc = ret_d.download(np.float32, (ROWS,)), disc_d.download(np.float32, (ROWS,))
        g = float(np.float32(GAMMA))
        assert (disc == 0).sum() >= 8 and (disc == np.float32(g * g * g)).sum() > ROWS // 2, "the chains are not 3 rows long"
        for k in ("ship", "tick_prev", "iaction", "px", "py", "reward"):             # the composite keeps r0's side
            assert np.array_equal(rows[k], mb["rows"][k]), k
        assert (rows["tick_next"] != mb["rows"]["tick_next"]).sum() > ROWS // 2
        mb["nstep"] = dict(rows=rows, rows_d=rows_d, bp_d=bp_d, bn_d=bn_d, ret_d=ret_d, disc_d=disc_d, ret=ret, disc=disc)
    return mb["nstep"]


@pytest.mark.parametrize("kind", ["one_step", "nstep"])
def test_targets_at_1500_rows(kind):
    """ofx_dqn_targets / ofx_dqn_targets_nstep (nstep = 3) on the 1500-row window: q_sa, p_sp, y_act, y_ptr equal to the
    call under OFX_OPT_TRUNK_FUSE = 2, y_act / y_ptr the same bits without the forward on `state`, and on the float64
    sample the definition of include/ofx.h formed from the float64 forwards."""
    mb = _minibatch()
    f64 = _mb_fp64(mb)
    if kind == "one_step":
        rows, args = mb["rows"], (mb["rows_d"], mb["prev"]["bits_d"], mb["next"]["bits_d"], None)
    else:
        ns = _nstep_window(mb)
        rows, args = ns["rows"], (ns["rows_d"], ns["bp_d"], ns["bn_d"], (ns["ret_d"], ns["disc_d"]))
    auto = _targets(mb, kind, ROWS, *args, True, 0, "stream", kind)
    split = _targets(mb, kind, ROWS, *args, True, 2, "split", kind)
    lean = _targets(mb, kind, ROWS, *args, False, 0, "stream", kind + ", targets only")
    lean_split = _targets(mb, kind, ROWS, *args, False, 2, "split", kind + ", targets only")
    names = ("q_sa", "p_sp", "y_act", "y_ptr")
    for k, name in enumerate(names):
        assert np.isfinite(auto[k]).all(), name
        assert auto[k].tobytes() == split[k].tobytes(), "%s: %s differs in rows %s" % (kind, name, np.flatnonzero(auto[k] != split[k])[:12])
    assert lean[0] is None and lean[1] is None and lean_split[0] is None and lean_split[1] is None
    for k in (2, 3):
        assert lean[k].tobytes() == auto[k].tobytes() and lean_split[k].tobytes() == auto[k].tobytes(), (kind, names[k])
    # the definition, in float64, on the sampled rows
    g = float(np.float32(GAMMA))
    worst, bad = np.zeros(4), []
    for i in f64["pick"]:
        i = int(i)
        r = rows[i]
        a0, h0 = f64["prev"][i]
        if kind == "one_step" or r["tick_next"] == mb["rows"]["tick_next"][i]:
            a1, h1 = f64["next"][i]
        else:                                   # the chain's last next_state: other maps, another head
            a1, h1 = _f64(args[2].download(np.uint32, (2, OB.WORDS), offset=i * ROW_BYTES), r["head_next"], mb["w"])
        if kind == "one_step":
            ret, disc = float(r["reward"]), (0.0 if r["done"] else g)
        else:
            ret, disc = float(ns["ret"][i]), float(ns["disc"][i])
        tol_a = TOL_ACT * max(1.0, float(np.abs(a0).max()), float(np.abs(a1).max()))
        tol_h = TOL_HEAT * max(float(np.abs(h0).max()), float(np.abs(h1).max()))
        want = (a0[r["iaction"]], h0[r["py"], r["px"]], ret + disc * a1.max(), ret + disc * h1.max())
        for k, tol in enumerate((tol_a, tol_h, tol_a, tol_h)):
            e = abs(float(auto[k][i]) - float(want[k])) / tol
            worst[k] = max(worst[k], e)
            if e > 1.0:
                bad.append((i, names[k], float(auto[k][i]), float(want[k]), tol))
    _report("targets_1500_" + kind, dict(zip(("q_sa_of_tol", "p_sp_of_tol", "y_act_of_tol", "y_ptr_of_tol"), map(float, worst)),
                                         rows=len(f64["pick"])))
    assert not bad, bad


def test_padded_targets_zero_pads_and_the_packed_bits():
    """ofx_replay_gather with batch = capacity: every arena holds fewer rows, so ship < 0 rows with empty maps sit among
    the N * CAP = 3072 rows.  Pads give exact zeros, every real row the bits of the packed (ofx_replay_gather_valid) call."""
    mb = _minibatch()
    b, total = mb["b"], mb["total"]
    rows_d, bp_d, bn_d = b.replay_gather_device(mb["slot"], CAP)
    b.sync()
    n = N * CAP
    rows = rows_d.download(b.TRANSITION_DTYPE, (n,))
    pads = rows["ship"] < 0
    assert n >= 1024 and pads.sum() == n - total and 0 < pads.sum() and pads.reshape(N, CAP).any(axis=1).all()
    for i in np.flatnonzero(pads)[:: max(1, int(pads.sum()) // 16)]:
        for buf in (bp_d, bn_d):
            assert not buf.download(np.uint32, (2, OB.WORDS), offset=int(i) * ROW_BYTES).any(), "pad row %d has bits set" % i
    padded = _targets(mb, "one_step", n, rows_d, bp_d, bn_d, None, True, 0, "stream", "padded")
    prow_d, pbp_d, pbn_d, got = b.replay_gather_valid(mb["slot"], mb["n_s"], CAP, 0, total)
    assert got == total
    assert np.array_equal(prow_d.download(b.TRANSITION_DTYPE, (total,)), rows[~pads])
    packed = _targets(mb, "one_step", total, prow_d, pbp_d, pbn_d, None, True, 0, "stream", "packed, all rows")
    for k, name in enumerate(("q_sa", "p_sp", "y_act", "y_ptr")):
        assert not padded[k][pads].any(), name                                   # exact zeros (+0 or -0: no bit set but the sign)
        assert padded[k][pads].tobytes() == np.zeros(int(pads.sum()), np.float32).tobytes(), name
        assert padded[k][~pads].tobytes() == packed[k].tobytes(), name
        # the window of the other tests is a prefix of the packed sequence
        assert packed[k][:ROWS].tobytes() == _targets_cached(mb)[k].tobytes(), name


def _targets_cached(mb):
    if "y1500" not in mb:
        mb["y1500"] = _targets(mb, "one_step", ROWS, mb["rows_d"], mb["prev"]["bits_d"], mb["next"]["bits_d"], None, True, 2,
                               "split", "one_step")
    return mb["y1500"]


# ---------------------------------------------------------------------------------------------- 3. synthetic maps
SYNTH_N = 3


def _synthetic(name):
    """(bits, vec8, probe, FUSE = 1 outputs, FUSE = 2 outputs, counters) of one pattern batch, cached."""
    key = ("synth", name)
    if key in _S:
        return _S[key]
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from oracle import pyoracle
    if "sb" not in _S:
        _S["sb"] = ArenaBatch(1, 2)                                  # forward_obs needs a handle, not its arenas
        w, _ = pyoracle.policy_init(6, trained_like=True)
        _S["sw"] = (w, DeviceBuffer(w.nbytes).upload(w))
    b, (w, w_d) = _S["sb"], _S["sw"]
    rs = np.random.RandomState(100 + sum(map(ord, name)))
    bits = OB.sweep_bits() if name == "sweep" else OB.pack_maps(OB.pattern_maps(name, SYNTH_N, rs))
    n = len(bits)
    vec = rs.uniform(-1, 1, (n, 8)).astype(np.float32)
    probe = rs.randint(0, 400, (n, 2)).astype(np.int32)
    b.sync()
    bits_d, vec_d, probe_d = DeviceBuffer(bits.nbytes).upload(bits), DeviceBuffer(vec.nbytes).upload(vec), DeviceBuffer(probe.nbytes).upload(probe)
    fused, st = _forward(b, w_d, n, bits_d.ptr, vec_d.ptr, probe_d.ptr, 1, "stream", "synthetic %s" % name)
    split, _ = _forward(b, w_d, n, bits_d.ptr, vec_d.ptr, probe_d.ptr, 2, "split", "synthetic %s" % name)
    _S[key] = dict(bits=bits, vec=vec, probe=probe, fused=fused, split=split, stats=st, w=w)
    return _S[key]


@pytest.mark.parametrize("name", OB.PATTERNS + ("sweep",))
def test_synthetic_maps_through_the_forced_sparse_trunk(name):
    """Maps an arena never produces, interleaved [n][2][5000], random heads: OFX_OPT_TRUNK_FUSE = 1 (the streaming trunk,
    sparse form forced on by vec8) equals OFX_OPT_TRUNK_FUSE = 2 in every output.  The sweep batch - observation k with
    one ship bit at (y = k, x = (7k + 3) % 400) and one laser bit at (y = (11k + 5) % 400, x = k) - puts a lone
    non-constant neighbourhood on every row and column: every 20-row step boundary of k_trunk12, every 16-pixel M-tile
    boundary, the tiles on the zero padding."""
    s = _synthetic(name)
    _assert_same(s["fused"], s["split"], "synthetic %s, fuse 1 vs 2" % name)
    run, total = s["stats"][:2]
    if name == "zero":
        assert run < total, (run, total)               # the interior M-tiles of an empty observation are all skipped
    if name == "sweep":
        assert run < total, (run, total)


def test_synthetic_maps_against_fp64():
    """The first observation of every pattern and three of the sweep against the float64 graph: all-zero, all-ones and
    frame-only maps among them."""
    worst = _Worst()
    todo = [(name, 0) for name in OB.PATTERNS] + [("sweep", k) for k in (0, 199, 399)]
    assert {"zero", "ones", "frame"} <= {t[0] for t in todo} and len(todo) >= 8
    for name, k in todo:
        s = _synthetic(name)
        a64, h64 = _f64(s["bits"][k], s["vec"][k], s["w"])
        worst.add(s["fused"], k, a64, h64, s["probe"][k], "%s[%d]" % (name, k))
    worst.verdict("forward_obs_synthetic")


# ---------------------------------------------------------------------------------------------- 4. probes on the frame
@pytest.mark.parametrize("legacy", [False, True])
def test_probe_on_the_heat_map_frame(legacy):
    """ptr_probe on the frame pixels of the heat map (the zero-padding corrections of the head's consumers' pass), next to
    them, on the arg-max and in the interior: == heat[y][x] of the map the live forward stored, ptr_max == heat.max(),
    ipointer == the live forward's - the same kernel family and arithmetic (tests/test_gpu_head_frame_argmax.py).  One
    batch of 1026 rows (6 observations x 171 probes: the streaming trunk) and one of 12; frame-seeking weights (the
    maximum itself sits on the frame) and one trained-like blob."""
    from ofighters_amd import ArenaBatch, DeviceBuffer, _native as nat
    from oracle import pyoracle
    n_ar, seed = 3, 77
    b = ArenaBatch(n_ar, M)
    b.set_option(nat.OPT_BILINEAR_LEGACY, int(legacy))
    b.spawn_random(seed)
    for t in range(30):
        b.bot_actions(["turret"] * (M // 2) + ["random"] * (M - M // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    ships = [(0, 2), (0, 5), (1, 0), (1, 7), (2, 3), (2, 4)]
    mask = np.zeros((n_ar, M), np.uint8)
    for g, i in ships:
        mask[g, i] = 1
    head, _ = b.observe_head()
    sm, lm = b.maps_host(nat.MAP_U8)
    obs_bits = OB.pack_maps(np.stack([sm, lm], 1))                                       # [arena][2][5000]
    corners, edges, near = OB.frame_probes()
    fixed = corners + edges + near
    rs = np.random.RandomState(5)
    per = 171
    S = len(ships)
    n_big, n_small = S * per, 12
    assert n_big >= 1024 and len(corners + edges) == n_small
    big_bits = np.repeat(np.stack([obs_bits[g] for g, _ in ships]), per, axis=0)
    big_vec = np.repeat(np.stack([head[g, i] for g, i in ships]).astype(np.float32), per, axis=0)
    small_obs = [k % S for k in range(n_small)]
    small_bits = np.stack([obs_bits[ships[s][0]] for s in small_obs])
    small_vec = np.stack([head[ships[s]] for s in small_obs]).astype(np.float32)
    small_probe = np.array(corners + edges, np.int32)
    b.sync()
    bb_d, bv_d, bp_d = DeviceBuffer(big_bits.nbytes).upload(big_bits), DeviceBuffer(big_vec.nbytes).upload(big_vec), DeviceBuffer(8 * n_big)
    sb_d, sv_d, sp_d = DeviceBuffer(small_bits.nbytes).upload(small_bits), DeviceBuffer(small_vec.nbytes).upload(small_vec), DeviceBuffer(8 * n_small).upload(small_probe)
    blobs = [(case, frame_weights(case, 40 + ci)) for ci, case in enumerate(FRAME_CASES)]
    blobs.append(("trained", pyoracle.policy_init(21, trained_like=True)[0]))
    seen = set()
    for case, w in blobs:
        live = b.policy_forward_host(w, ship_mask=mask, want_heat=True)
        w_d = DeviceBuffer(w.nbytes).upload(w)
        heats = [live["heat"][g, i] for g, i in ships]
        probe = np.zeros((S, per, 2), np.int32)
        for s, heat in enumerate(heats):
            k = int(np.argmax(heat))
            if case != "trained":
                seen.update(where(k // 400, k % 400))
                assert case in where(k // 400, k % 400), "the weights of case %r did not put the maximum on the frame: (y %d, x %d)" % (case, k // 400, k % 400)
            probe[s, :len(fixed)] = fixed
            probe[s, len(fixed)] = (k % 400, k // 400)
            probe[s, len(fixed) + 1:] = rs.randint(1, 399, (per - len(fixed) - 1, 2))
        b.sync()
        bp_d.upload(probe)
        big, _ = _forward(b, w_d, n_big, bb_d.ptr, bv_d.ptr, bp_d.ptr, 0, "stream", "probes, %s" % case)
        small, _ = _forward(b, w_d, n_small, sb_d.ptr, sv_d.ptr, sp_d.ptr, 0, "split", "probes, %s" % case)
        flat = probe.reshape(n_big, 2)
        for out, obs_of, pr in ((big, np.repeat(np.arange(S), per), flat), (small, small_obs, small_probe)):
            want_probe = np.array([heats[s][y, x] for s, (x, y) in zip(obs_of, pr)], np.float32)
            want_max = np.array([heats[s].max() for s in obs_of], np.float32)
            want_ptr = np.array([live["ipointer"][ships[s]] for s in obs_of], np.int32)
            want_act = np.array([live["act"][ships[s]] for s in obs_of], np.float32)
            bad = np.flatnonzero(out["ptr_probe"] != want_probe)
            assert bad.size == 0, "%s legacy %d: ptr_probe != heat[y][x] at probes (x, y) %s: %r != %r" % (
                case, legacy, pr[bad[:8]].tolist(), out["ptr_probe"][bad[:8]], want_probe[bad[:8]])
            assert np.array_equal(out["ptr_max"], want_max), (case, legacy)
            assert np.array_equal(out["ipointer"], want_ptr), (case, legacy)
            assert np.array_equal(out["act"], want_act), (case, legacy)
    assert seen >= set(FRAME_CASES), seen
    b.close()


# ---------------------------------------------------------------------------------------------- 5. DeviceTrainer
@pytest.mark.parametrize("prioritized,n_step", [(False, 1), (True, 3)])
def test_device_trainer_replay_at_a_production_window(prioritized, n_step):
    """DeviceTrainer.replay() with fit_batch = 1536, twice from identical state: OFX_OPT_TRUNK_FUSE auto (the targets come
    out of the streaming trunk) and 2.  The targets are equal and the fit is bit-reproducible, so the losses, the updated
    blob and both Adam moments are the same bits - uniform replay, and prioritized replay with 3-step returns (there the
    written-back priorities too)."""
    from ofighters_amd import ArenaBatch
    from ofighters_amd.trainer import DeviceTrainer
    from oracle import pyoracle
    fit = 1536
    b = ArenaBatch(N, M)
    w, _ = pyoracle.policy_init(4, trained_like=True)
    tr = DeviceTrainer(b, w, learning_rate=1e-3, batch_size=CAP, memory_size=CAP, fit_batch=fit, prioritized=prioritized,
                       n_step=n_step)
    b.spawn_random(SEED)
    _play(b, *_capture_buffers(N))
    zeros = np.zeros_like(w)
    runs = []
    for fuse, path in ((0, "stream"), (2, "split")):
        b.sync()
        tr.weights.upload(w); tr.adam_m.upload(zeros); tr.adam_v.upload(zeros)
        tr.fit_steps, tr.draws, tr.losses = 0, 0, []
        if prioritized:
            b.replay_prioritize(tr.per_alpha, tr.per_eps)            # every mass and the running maximum back to 1.0
        with _Options(b, fuse) as o:
            loss = tr.replay()
        assert loss is not None and np.isfinite(loss).all() and tr.fit_steps == 1
        _check_path(o.stats, fit, path, "DeviceTrainer.replay, fuse %d" % fuse)  # one forward (next_state) of 1536 rows
        b.sync()
        runs.append(dict(loss=loss, w=tr.weights_host(), m=tr.adam_m.download(np.float32, w.shape),
                         v=tr.adam_v.download(np.float32, w.shape),
                         prio=[b.replay_priorities(a) for a in range(N)] if prioritized else []))
    a, c = runs
    assert np.isfinite(a["w"]).all() and np.abs(a["w"] - w).max() > 0 and np.abs(a["m"]).max() > 0
    assert a["loss"] == c["loss"], (a["loss"], c["loss"])
    for k in ("w", "m", "v"):
        assert a[k].tobytes() == c[k].tobytes(), k
    for pa, pc in zip(a["prio"], c["prio"]):
        assert pa.tobytes() == pc.tobytes()
    if prioritized:
        assert any((p != 1.0).any() for p in a["prio"])              # priorities were written back
    b.close()
