"""The four TD target entries (ofx_dqn_targets, _nstep, _double, _soft) where their contracts in include/ofx.h say they
coincide, and against the one exact float32 statement of their arithmetic (tests/td_oracle.py) fed with the host results
of ofx_policy_forward_obs on the same bits - the library is reproducible to the bit, so the forwards the entries ran
inside gave those values.

n = 1, 255 and 257 rows: one row, the last thread of the targets kernel's 256-thread block, and one past it.  The rows are
synthetic ofx_transition records over random sparse bit maps: a padding row (ship < 0), done rows, both actions, pointers
outside [0, 399] (the entries clamp them) and rewards of either sign; the weights are synthetic(7), the second blob of the
Double DQN case synthetic(8)."""
import numpy as np
import pytest

from tests import ddqn_oracle, td_oracle
from tests.obs_batches import WORDS

pytestmark = pytest.mark.gpu

GAMMA = 0.9
SIZES = (1, 255, 257)
NAMES = ("q_sa", "p_sp", "y_act", "y_ptr")
_S = {}


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    if "b" in _S:
        _S["b"].close()
    _S.clear()


def _handle():
    if "b" not in _S:
        from ofighters_amd import ArenaBatch, DeviceBuffer
        from ofighters_amd.agents.policy_weights import synthetic
        _S["b"] = ArenaBatch(1, 2)                                   # the entries need a handle, not its arenas
        for k, seed in (("w", 7), ("w2", 8)):
            w = synthetic(seed)
            _S[k] = DeviceBuffer(w.nbytes).upload(w)
    return _S["b"]


def _sparse_bits(rs, n):
    """[n][2][WORDS] uint32: about 60 random pixels set per map."""
    bits = np.zeros((n, 2, WORDS), np.uint32)
    for i in range(n):
        for m in range(2):
            p = rs.randint(0, 32 * WORDS, 60)
            np.bitwise_or.at(bits[i, m], p >> 5, np.uint32(1) << (p & 31).astype(np.uint32))
    return bits


def _rows(rs, n, dtype):
    rows = np.zeros(n, dtype)
    rows["tick_prev"], rows["tick_next"] = np.arange(n), np.arange(n) + 1
    rows["ship"] = rs.randint(0, 8, n)
    rows["iaction"] = rs.randint(0, 2, n)
    rows["px"], rows["py"] = rs.randint(-40, 440, n), rs.randint(-40, 440, n)
    rows["reward"] = rs.randint(-3, 4, n)
    rows["done"] = rs.rand(n) < 0.25
    rows["head_prev"], rows["head_next"] = rs.uniform(-1, 1, (n, 8)), rs.uniform(-1, 1, (n, 8))
    if n == 1:                                   # the one row: a live, rewarded step with its pointer off the map
        rows["iaction"], rows["done"], rows["reward"], rows["px"], rows["py"] = 1, 0, 2, -7, 431
    else:
        rows["ship"][n // 2] = -1                # a padding row in the middle; the first and the last row done
        rows["done"][[0, n - 1]], rows["done"][1] = 1, 0
        rows["iaction"][[0, 1]] = 0, 1
        rows["px"][[2, 3]], rows["py"][[2, 3]] = (-1, 400), (400, -1)
        assert len(set(rows["iaction"])) == 2 and (rows["px"] > 399).any() and (rows["py"] < 0).any()
    return rows


def _case(n):
    """The rows of size n on the device, and every entry's result and every forward, computed once."""
    if n in _S:
        return _S[n]
    from ofighters_amd import DeviceBuffer, _native as nat
    b = _handle()
    L, h, w, w2 = nat.lib(), b.handle, _S["w"].ptr, _S["w2"].ptr
    rs = np.random.RandomState(1000 + n)
    rows = _rows(rs, n, b.TRANSITION_DTYPE)
    up = lambda a: DeviceBuffer(a.nbytes).upload(np.ascontiguousarray(a))
    ret = rs.uniform(-3, 3, n).astype(np.float32)
    disc = np.where(rs.rand(n) < 0.25, 0, np.float32(GAMMA) ** rs.randint(1, 4, n)).astype(np.float32)
    rows_d, bp_d, bn_d, ret_d, disc_d = up(rows), up(_sparse_bits(rs, n)), up(_sparse_bits(rs, n)), up(ret), up(disc)

    def call(fn, head, tail=()):
        out = [DeviceBuffer(4 * n) for _ in NAMES]
        nat.check(fn(h, *head, n, rows_d.ptr, bp_d.ptr, bn_d.ptr, *tail, *[o.ptr for o in out]))
        b.sync()
        return [o.download(np.float32, (n,)) for o in out]

    c = dict(rows=rows, ret=ret, disc=disc, pad=rows["ship"] < 0)
    one, nstep = (GAMMA, None, None), (GAMMA, ret_d.ptr, disc_d.ptr)
    c["plain"] = call(L.ofx_dqn_targets, (w,), (GAMMA,))
    c["nstep"] = call(L.ofx_dqn_targets_nstep, (w,), nstep[1:])
    c["double_self"] = call(L.ofx_dqn_targets_double, (w, w), one)
    c["double_self_nstep"] = call(L.ofx_dqn_targets_double, (w, w), nstep)
    c["double"] = call(L.ofx_dqn_targets_double, (w, w2), one)
    c["double_nstep"] = call(L.ofx_dqn_targets_double, (w, w2), nstep)
    c["soft0"] = call(L.ofx_dqn_targets_soft, (w,), one + (0.0, 0.0, 0.0, 0.0))
    c["soft0_nstep"] = call(L.ofx_dqn_targets_soft, (w,), nstep + (0.0, 0.0, 0.0, 0.0))
    # the forwards, as the entries unpack the rows: zero heads for a padding row, the pointer clamped to the map
    keep = ~c["pad"][:, None]
    probe = np.where(keep, np.stack([np.clip(rows["px"], 0, 399), np.clip(rows["py"], 0, 399)], 1), 0).astype(np.int32)
    vp_d, vn_d = up(np.where(keep, rows["head_prev"], 0).astype(np.float32)), up(np.where(keep, rows["head_next"], 0).astype(np.float32))
    probe_d = up(probe)
    c["prev"] = b.policy_forward_obs(w, n, bp_d.ptr, vp_d.ptr, probe_d.ptr)
    c["next"] = b.policy_forward_obs(w, n, bn_d.ptr, vn_d.ptr)
    sel_d = up(c["next"]["ipointer"])                # the target network is probed where the online one points
    c["next_w2"] = b.policy_forward_obs(w2, n, bn_d.ptr, vn_d.ptr, sel_d.ptr)
    _S[n] = c
    return c


def _same(got, want, what):
    for k, name in enumerate(NAMES):
        assert np.isfinite(got[k]).all(), (what, name)
        assert got[k].tobytes() == want[k].tobytes(), "%s: %s differs in rows %s" % (what, name, np.flatnonzero(got[k] != want[k])[:12])


def _current(c):
    """q_sa / p_sp as every entry must report them: the forward on `state`, zeros for a padding row."""
    act, a = c["prev"]["act"], (c["rows"]["iaction"] != 0).astype(np.intp)
    zero = np.float32(0)
    return [np.where(c["pad"], zero, act[np.arange(len(a)), a]), np.where(c["pad"], zero, c["prev"]["ptr_probe"])]


@pytest.mark.parametrize("n", SIZES)
def test_plain_and_nstep_equal_the_float32_oracle(n):
    c = _case(n)
    act = c["next"]["act"]
    v_act, v_ptr = np.maximum(act[:, 0], act[:, 1]), c["next"]["ptr_max"]
    _same(c["plain"], _current(c) + list(td_oracle.targets(c["rows"], GAMMA, v_act, v_ptr)), "one-step, n %d" % n)
    _same(c["nstep"], _current(c) + list(td_oracle.targets(c["rows"], None, v_act, v_ptr, c["ret"], c["disc"])), "n-step, n %d" % n)
    if n > 1:
        assert c["pad"].sum() == 1 and all(not o[c["pad"]].any() for o in c["plain"] + c["nstep"])
        live = ~c["pad"]
        assert (c["plain"][2][live] != c["nstep"][2][live]).any() and (c["rows"]["done"][live] != 0).any()


@pytest.mark.parametrize("n", SIZES)
def test_double_with_its_own_blob_as_target_is_plain(n):
    c = _case(n)
    _same(c["double_self"], c["plain"], "double(w, w) vs plain, n %d" % n)
    _same(c["double_self_nstep"], c["nstep"], "double(w, w) vs n-step, n %d" % n)


@pytest.mark.parametrize("n", SIZES)
def test_double_with_a_second_blob_equals_the_oracle_on_the_two_forwards(n):
    c = _case(n)
    sel, tgt = c["next"]["iaction"], c["next_w2"]
    for key, ret, disc in (("double", None, None), ("double_nstep", c["ret"], c["disc"])):
        want = ddqn_oracle.targets_double(c["rows"], GAMMA, ret, disc, sel, tgt["act"], tgt["ptr_probe"])
        _same(c[key], _current(c) + list(want), "%s, n %d" % (key, n))
    live = ~c["pad"]
    assert (c["double"][2][live] != c["plain"][2][live]).any(), "the second blob evaluates like the first"


@pytest.mark.parametrize("n", SIZES)
def test_soft_at_zero_temperatures_without_the_bonus_is_plain(n):
    c = _case(n)
    _same(c["soft0"], c["plain"], "soft(0, 0, 0) vs plain, n %d" % n)
    _same(c["soft0_nstep"], c["nstep"], "soft(0, 0, 0) vs n-step, n %d" % n)
