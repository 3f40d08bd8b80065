"""OFX_OPT_TRUNK_SPARSE is tri-state: a handle that never set it runs the exact sparse streaming trunk (k_trunk12<., true>)
without counters, 1 adds the counters of ofx_policy_trunk_stats, 0 asks for the dense kernel (the reference here).  Every
output is compared with ==; the counters are compared with the CPU model of tests/trunk_sparse_model.py, exactly.
OFX_OPT_TRUNK_FUSE = 1 throughout: the streaming trunk at every batch size."""
import numpy as np
import pytest

from tests import trunk_sparse_model as TM

pytestmark = pytest.mark.gpu

M = 2
_W = {}


def _weights():
    if "w" not in _W:
        from oracle import pyoracle
        _W["w"] = pyoracle.policy_init(7, trained_like=True)[0]
    return _W["w"]


def _rollout(N, seed, ticks):
    from ofighters_amd import ArenaBatch, _native as nat
    b = ArenaBatch(N, M)
    b.spawn_random(seed)
    for t in range(ticks):
        b.bot_actions(["turret"] * (M // 2) + ["random"] * (M - M // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    return b


def _same(got, ref, what):
    for k in ref:
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


def _model_counts(b):
    from ofighters_amd import _native as nat
    marks = TM.pair_marks(TM.unpack(*b.maps_host(nat.MAP_BITS)))
    run = int(TM.tiles_run(marks).sum())
    trun, ttotal = TM.table_passes(marks)
    return marks, (run, b.N * TM.STEPS * TM.NT, trun, ttotal)


def _three_forms(b, what, heat=True):
    """never set / 0 / 1 on one handle: outputs ==, counters only with 1; returns the counters of the forward with 1."""
    from ofighters_amd import _native as nat
    w = _weights()
    assert b.policy_trunk_stats() == (0, 0, 0, 0)
    default = b.policy_forward_host(w, want_heat=heat)
    assert b.policy_trunk_stats() == (0, 0, 0, 0), "a handle that never set the option counts nothing"
    b.set_option(nat.OPT_TRUNK_SPARSE, 0)
    dense = b.policy_forward_host(w, want_heat=heat)
    assert b.policy_trunk_stats() == (0, 0, 0, 0)
    b.set_option(nat.OPT_TRUNK_SPARSE, 1)
    counted = b.policy_forward_host(w, want_heat=heat)
    st = b.policy_trunk_stats()
    _same(default, dense, what + ": never set vs 0")
    _same(counted, dense, what + ": 1 vs 0")
    return st


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2, 5, 40])
def test_default_equals_dense(N, mode):
    """Mid-episode rollouts of 1, 2, 5 and 40 arenas x 2 ships, fp32 and both 16-bit operand modes: a fresh handle's
    forward, heat map included, == the dense kernel's, and so is the counting form; the counters are the model's."""
    from ofighters_amd import _native as nat
    b = _rollout(N, seed=40 + N, ticks=30)
    b.set_option(nat.OPT_POLICY_BF16, mode)
    st = _three_forms(b, "N %d mode %d" % (N, mode))
    marks, want = _model_counts(b)
    print("N %d mode %d: counters %r, model %r" % (N, mode, st, want))
    assert want[1] == N * 20 * 63
    assert st == want
    b.close()


# p1 columns and rows on which marks have to fall: tile starts, the row-pair crossing 192 | 0, both alignments of the
# alternating row pairs, the step boundaries, the four corners
P1_COLS = (0, 1, 7, 8, 15, 16, 17, 183, 184, 191, 192, 198, 199)
P1_ROWS = (0, 1, 9, 10, 11, 189, 190, 191, 198, 199)


def test_placements_on_tile_and_step_boundaries():
    """Fresh spawns (ships only), the two ships of an arena moved with set_ships onto every combination of the image
    coordinates 2 c (c in P1_COLS + P1_ROWS), 399 and 400 on both axes; the last arena has both ships inside one interior
    40 x 40 block.  Outputs == dense, counters == the model, per placement batch."""
    from ofighters_amd import ArenaBatch, _native as nat
    coords = sorted({2 * c for c in P1_COLS + P1_ROWS} | {399, 400})
    xy = np.array([(x, y) for x in coords for y in coords])
    xy = np.concatenate([xy, xy[:len(xy) % 2]])                                  # two ships per arena
    N = len(xy) // 2 + 1
    x = np.concatenate([xy[:, 0], [185, 210]]).reshape(N, M)
    y = np.concatenate([xy[:, 1], [190, 215]]).reshape(N, M)
    b = ArenaBatch(N, M)
    b.spawn_random(11)
    b.set_ships(x=x, y=y)
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    st = _three_forms(b, "placements", heat=False)                         # 201 arenas: the heat maps are compared above
    marks, want = _model_counts(b)
    hit_rows, hit_cols = marks.any(axis=(0, 2)), np.repeat(marks.any(axis=(0, 1)), 2)
    assert hit_rows[list(P1_ROWS)].all() and hit_cols[list(P1_COLS)].all()
    for cy in (0, 199):                                                          # the four corners
        for cp in (0, 99):
            assert marks[:, cy, cp].any(), (cy, cp)
    print("placements: counters %r, model %r" % (st, want))
    assert st == want
    # the packed arena alone: its marks stay inside the block's neighbourhood, and every tile it runs beyond the forced
    # ones is there
    one = TM.tiles_run(marks[-1:])
    floor = TM.tiles_run(np.zeros_like(marks[-1:]))
    assert marks[-1].any() and not marks[-1, :80].any() and not marks[-1, 125:].any()
    # 45 p1 rows -> at most 24 row pairs, 45 + 18 columns -> at most 5 tiles each: under a tenth of the image's 1260
    assert floor.sum() == 182 and 0 < (one & ~floor).sum() < 126
    b.close()


def test_option_life_cycle():
    """Never set: no counters exist.  1: they count.  0: dense, and they stay silent.  1 again: they count again.  The
    forward is == in all four states."""
    from ofighters_amd import _native as nat
    b = _rollout(5, seed=3, ticks=20)
    w = _weights()
    assert b.policy_trunk_stats() == (0, 0, 0, 0)
    fresh = b.policy_forward_host(w, want_heat=True)
    assert b.policy_trunk_stats() == (0, 0, 0, 0)
    b.set_option(nat.OPT_TRUNK_SPARSE, 1)
    one = b.policy_forward_host(w, want_heat=True)
    st = b.policy_trunk_stats()
    assert st[1] == 5 * 20 * 63 and 0 < st[0] < st[1] and 0 < st[2] < st[3]
    assert b.policy_trunk_stats() == (0, 0, 0, 0)                                # reading resets
    b.set_option(nat.OPT_TRUNK_SPARSE, 0)
    dense = b.policy_forward_host(w, want_heat=True)
    assert b.policy_trunk_stats() == (0, 0, 0, 0)
    b.set_option(nat.OPT_TRUNK_SPARSE, 1)
    again = b.policy_forward_host(w, want_heat=True)
    assert b.policy_trunk_stats() == st
    for name, got in (("never set", fresh), ("1", one), ("1 again", again)):
        _same(got, dense, name)
    b.close()
