"""The (iaction, ipointer) that ofx_policy_forward / ofx_policy_explore keep for a null result pointer belong to the
handle, not to the transient scratch block: they survive every other call that uses that block.

2 arenas x 2 ships is the smallest shape with the hazard: the per-layer trunk form, whose workspace (about 3.5 MB,
mostly the pooled conv1 activation) a forward on 3 stored observations outgrows - another layout in a re-allocated
block, where the results used to sit at an offset that depended on both.  ofx_agents_first_done and the scratch MLP
wrote at byte 0 of the same block."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M, SEED, TICK = 2, 2, 0x0F160021, 7
S = N * M
ACTION_BYTES = 12   # struct ofx_action


def _intrude(b, dw):
    """Every other user of the handle's scratch block, between the forward and the packing of its results."""
    from ofighters_amd import DeviceBuffer, _native as nat
    lib = nat.lib()
    rs = np.random.RandomState(5)
    bits = (rs.randint(0, 1 << 32, (3, 2, 5000), dtype=np.uint64) & rs.randint(0, 1 << 32, (3, 2, 5000), dtype=np.uint64)
            & rs.randint(0, 1 << 32, (3, 2, 5000), dtype=np.uint64)).astype(np.uint32)
    vec = rs.uniform(0, 400, (3, 8)).astype(np.float32)
    dbits, dvec = DeviceBuffer(bits.nbytes).upload(bits), DeviceBuffer(vec.nbytes).upload(vec)
    # null outputs: its own throw-away slots, never the handle's results
    nat.check(lib.ofx_policy_forward_obs(b.handle, dw.ptr, 3, dbits.ptr, dvec.ptr, None, None, None, None, None, None))
    seen = DeviceBuffer(S).upload(np.zeros(S, np.uint8))
    assert b.agents_first_done(None, seen) >= 0
    layers = np.array([8, 4], np.int32)
    w, bias, x = rs.uniform(-1, 1, 32), rs.uniform(-1, 1, 4), rs.uniform(-1, 1, (S, 8))
    dws, dbs, dx = DeviceBuffer(w.nbytes).upload(w), DeviceBuffer(bias.nbytes).upload(bias), DeviceBuffer(x.nbytes).upload(x)
    dy, da = DeviceBuffer(8 * S * 4), DeviceBuffer(4 * S)
    nat.check(lib.ofx_scratch_feed(b.handle, layers.ctypes.data_as(C.c_void_p), 2, dws.ptr, dbs.ptr, dx.ptr, S, dy.ptr, da.ptr))
    b.sync()


@pytest.mark.parametrize("explore", [False, True])
def test_handle_results_survive_other_users_of_the_scratch_block(explore):
    from ofighters_amd import ArenaBatch, DeviceBuffer
    from ofighters_amd.agents.policy_weights import synthetic
    b = ArenaBatch(N, M)
    try:
        b.spawn_random(SEED)
        for t in range(5):
            b.bot_actions(["random"] * M, SEED, tick=t)
            b.step(actions_ptr=b._actions.ptr)
        w = synthetic()
        dw = DeviceBuffer(w.nbytes).upload(w)

        def packed(iaction_ptr=None, ipointer_ptr=None):
            out = DeviceBuffer(ACTION_BYTES * S)
            b.policy_actions(out.ptr, iaction_ptr, ipointer_ptr)
            b.sync()
            return out.download(np.uint8, (S, ACTION_BYTES))

        b.policy_forward(dw.ptr)                                   # null result pointers: kept by the handle
        if explore:
            b.policy_explore(1.0, SEED, tick=TICK)                  # eps = 1: every ship's result is replaced
        first = packed()
        _intrude(b, dw)
        second = packed()
        # the same forward (the state has not moved) into buffers of the caller
        di, dp = DeviceBuffer(4 * S), DeviceBuffer(8 * S)
        b.policy_forward(dw.ptr, None, None, di.ptr, dp.ptr)
        if explore:
            b.policy_explore(1.0, SEED, tick=TICK, iaction_ptr=di.ptr, ipointer_ptr=dp.ptr)
        explicit = packed(di.ptr, dp.ptr)
        assert first.tobytes() == second.tobytes()
        assert first.tobytes() == explicit.tobytes()
        assert first[:, 10].any(), "no live ship: the packed actions say nothing"   # ofx_action.valid
    finally:
        b.close()
