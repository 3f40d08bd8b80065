"""The sparse streaming conv3 (k_conv3_stream<., true>): it runs exactly when the sparse k_trunk12 made its input, takes that
kernel's p2 marks and stores conv3's constant for the M-tiles whose window is unmarked and off the padding.  Every output
of the forward - act, iaction, ipointer, heat and the trunk features - is compared with == against OFX_OPT_TRUNK_SPARSE = 0
(the dense k_trunk12 + dense conv3 pair); the counters of ofx_policy_trunk_stats3 are compared with the CPU model of
tests/conv3_sparse_model.py, exactly.  OFX_OPT_TRUNK_FUSE = 1 throughout: the streaming kernels at every batch size."""
import ctypes as C

import numpy as np
import pytest

from tests import conv3_sparse_model as CM
from tests import trunk_sparse_model as TM

pytestmark = pytest.mark.gpu

M = 2
_W = {}


def _weights():
    if "w" not in _W:
        from oracle import pyoracle
        _W["w"] = pyoracle.policy_init(7, trained_like=True)[0]
    return _W["w"]


def _rollout(N, seed, ticks, m=M):
    from ofighters_amd import ArenaBatch, _native as nat
    b = ArenaBatch(N, m)
    b.spawn_random(seed)
    for t in range(ticks):
        b.bot_actions(["turret"] * (m // 2) + ["random"] * (m - m // 2), seed, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    return b


def _forward(b, heat):
    out = b.policy_forward_host(_weights(), want_heat=heat)
    out["features"] = b.policy_trunk_features()
    return out


def _same(got, ref, what):
    for k in ref:
        assert got[k].tobytes() == ref[k].tobytes(), (what, k)


def _forms(b, what, heat=True):
    """never set / 0 / 1 on one handle: every output == the dense pair's; returns conv3's counters of the forward with 1."""
    from ofighters_amd import _native as nat
    assert b.policy_trunk_stats3() == (0, 0)
    default = _forward(b, heat)
    assert b.policy_trunk_stats3() == (0, 0), "a handle that never set the option counts nothing"
    b.set_option(nat.OPT_TRUNK_SPARSE, 0)
    dense = _forward(b, heat)
    assert b.policy_trunk_stats3() == (0, 0)
    b.set_option(nat.OPT_TRUNK_SPARSE, 1)
    counted = _forward(b, heat)
    st = b.policy_trunk_stats3()
    assert b.policy_trunk_stats3() == (0, 0)                                     # reading resets
    assert sorted(dense) == sorted(["act", "iaction", "ipointer", "features"] + (["heat"] if heat else []))
    assert np.isfinite(dense["features"]).all() and dense["features"].any()
    _same(default, dense, what + ": never set vs 0")
    _same(counted, dense, what + ": 1 vs 0")
    return st


def _model(b):
    from ofighters_amd import _native as nat
    return CM.counts(TM.unpack(*b.maps_host(nat.MAP_BITS)))


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("N", [1, 2, 5, 40])
def test_equals_dense(N, mode):
    """Mid-episode rollouts of 1, 2, 5 and 40 arenas x 2 ships, fp32 and both 16-bit operand modes."""
    from ofighters_amd import _native as nat
    b = _rollout(N, seed=60 + N, ticks=30)
    b.set_option(nat.OPT_POLICY_BF16, mode)
    st = _forms(b, "N %d mode %d" % (N, mode))
    want = _model(b)
    print("N %d mode %d: conv3 counters %r, model %r" % (N, mode, st, want))
    assert want[1] == N * 5 * 63 and 0 < want[0] < want[1]
    assert st == want
    b.close()


def test_more_images_than_workgroups():
    """300 arenas: a workgroup walks several images, the marks of the next image's first step arrive under the last step
    of this one."""
    b = _rollout(300, seed=19, ticks=25)
    st = _forms(b, "300 arenas", heat=False)
    assert st == _model(b)
    b.close()


@pytest.mark.parametrize("legacy", [0, 1])
def test_equals_dense_both_bilinear_conventions(legacy):
    from ofighters_amd import _native as nat
    b = _rollout(5, seed=71, ticks=25)
    b.set_option(nat.OPT_BILINEAR_LEGACY, legacy)
    st = _forms(b, "legacy %d" % legacy)
    assert st == _model(b)
    b.close()


def _kill_all(b):
    from ofighters_amd import _native as nat
    dead = np.zeros((b.N, b.M), np.uint8)
    b.sync()
    nat.check(nat.lib().ofx_memcpy_h2d(nat.lib().ofx_device_ptr(b._h, nat.F_SHIP_ALIVE), dead.ctypes.data_as(C.c_void_p), dead.nbytes))


def test_empty_map_runs_only_forced_tiles():
    """No playable ship, no laser: both maps are empty, p2 is conv2's constant away from the borders and conv3 runs its forced
    tiles and the windows next to conv2's border tiles - some, not all."""
    from ofighters_amd import ArenaBatch, _native as nat
    b = ArenaBatch(3, M)
    b.spawn_random(5)
    _kill_all(b)
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    bits = TM.unpack(*b.maps_host(nat.MAP_BITS))
    assert not bits.any()
    run, total = _forms(b, "empty map")
    print("empty map: conv3 counters %r, model %r" % ((run, total), CM.counts(bits)))
    assert total == 3 * 5 * 63 and 0 < run < total
    assert (run, total) == CM.counts(bits)
    b.close()


def _c(p2):
    """image coordinate of the centre of p2 pixel p2 (a p2 pixel is 4 x 4 image cells)."""
    return 4 * p2 + 2


# (x, y) image positions of the single-ship scenes, both ships of an arena on the same spot
SCENES = (
    [(x, y) for x in (0, 399) for y in (0, 399)]                                 # the corners
    + [(200, 0), (200, 399), (0, 200), (399, 200), (400, 400)]                   # the edge midpoints, the far corner cell
    + [(200, _c(r)) for r in (19, 20, 21, 39, 40)]                               # conv3's step seams (20 rows per step, 22-row tiles)
    + [(_c(r), 200) for r in (19, 20, 21, 39, 40)]
    + [(_c(c), 120) for c in (15, 16, 17)] + [(120, _c(c)) for c in (15, 16, 17)]  # the first tile boundary
    # the flat enumeration crosses row pairs in tiles 6, 12, 18, 24 (pixels 96 | 0, 92 | 0, 88 | 0, 84 | 0): ships on both sides
    + [(_c(c), _c(r)) for c in (97, 2, 93, 89, 85, 83, 8) for r in (1, 3, 5, 7, 30)]
    # every alignment of a ship's edge against conv2's 8-pixel and conv3's 16-pixel tiles and against the 5-row / 20-row steps:
    # 32 consecutive image columns at one row, 40 consecutive image rows at one column (a mark one column or one row off
    # leaves the ship's first or last non-constant p2 pixel outside every marked window at some of them)
    + [(100 + i, 210) for i in range(32)] + [(210, 100 + i) for i in range(40)]
)


def test_single_ship_scenes():
    """One ship per arena at each corner, edge midpoint, on conv3's step seams, on the tile boundary columns 15 / 16 / 17 and
    on the columns where the flat M-tile enumeration passes from one row pair to the next: outputs == dense, counters ==
    the model, and every scene's marks are where the ship is."""
    from ofighters_amd import ArenaBatch, _native as nat
    xy = np.array(SCENES)
    N = len(xy)
    b = ArenaBatch(N, M)
    b.spawn_random(13)
    b.set_ships(x=np.repeat(xy[:, :1], M, axis=1), y=np.repeat(xy[:, 1:], M, axis=1))
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    st = _forms(b, "scenes", heat=False)                                         # the heat maps are compared in the other tests
    bits = TM.unpack(*b.maps_host(nat.MAP_BITS))
    assert bits.any(axis=(1, 2)).all()
    want = CM.counts(bits)
    marks2 = CM.p2_marks(TM.tiles_run(TM.pair_marks(bits)))
    rows, cols = marks2.any(axis=2), marks2.any(axis=1)
    for r in (19, 20, 21, 39, 40):
        assert rows[:, r].any() and cols[:, r].any()
    for c in (15, 16, 17, 97, 2, 83):
        assert cols[:, c].any() or rows[:, c].any()
    floor = CM.tiles_run(np.zeros_like(marks2))
    per_scene = (CM.tiles_run(marks2) & ~floor).sum(axis=(1, 2))
    assert marks2.any(axis=(1, 2)).all() and (per_scene > 0).any() and (per_scene < 63).all()  # a ship is a few tiles, not the image
    print("scenes: conv3 counters %r, model %r" % (st, want))
    assert st == want
    b.close()


def test_brawl_in_a_corner():
    """8 ships packed into one corner, shooting for 12 ticks: everything non-constant there, nothing elsewhere."""
    from ofighters_amd import ArenaBatch, _native as nat
    rs = np.random.RandomState(5)
    b = ArenaBatch(4, 8)
    b.spawn_random(3)
    b.set_ships(x=rs.randint(0, 40, (4, 8)), y=rs.randint(360, 401, (4, 8)))
    for t in range(12):
        b.bot_actions(["turret"] * 8, 5, tick=t)
        b.step(actions_ptr=b._actions.ptr)
    b.set_option(nat.OPT_TRUNK_FUSE, 1)
    st = _forms(b, "brawl")
    want = _model(b)
    print("brawl: conv3 counters %r, model %r" % (st, want))
    assert 0.2 * want[1] < want[0] < want[1]
    assert st == want
    b.close()
