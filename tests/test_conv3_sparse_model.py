"""CPU checks of tests/conv3_sparse_model.py (the model the GPU counters of ofx_policy_trunk_stats3 are held to): the marks
against a per-pixel restatement, the forced tiles of an empty map, and that the scenes of tests/test_gpu_conv3_sparse.py
leave the counters room on both sides (run < total on the empty map, run > 0.2 total on a packed corner)."""
import numpy as np

from tests import conv3_sparse_model as CM
from tests import trunk_sparse_model as TM


def _discs(centres, radius=6):
    bits = np.zeros((1, TM.SIDE, TM.SIDE), bool)
    yy, xx = np.mgrid[:TM.SIDE, :TM.SIDE]
    for (y, x) in centres:
        bits[0] |= (yy - y) ** 2 + (xx - x) ** 2 <= radius ** 2
    return bits


def test_marks_are_the_pixels_of_the_tiles_that_ran():
    rs = np.random.RandomState(1)
    run2 = rs.rand(3, TM.STEPS, TM.NT) < 0.3
    got = CM.p2_marks(run2)
    want = np.zeros((3, 100, 100), bool)
    for step in range(TM.STEPS):
        for T in range(TM.NT):
            for px in range(16 * T, min(16 * T + 16, 1000)):                     # conv2 pixels of the tile: row pair, column
                rp, x = divmod(px, 200)
                want[:, 5 * step + rp, x // 2] |= run2[:, step, T]
    assert np.array_equal(got, want)


def test_empty_map_runs_only_the_forced_tiles():
    empty = np.zeros((1, TM.SIDE, TM.SIDE), bool)
    run2 = TM.tiles_run(TM.pair_marks(empty))
    run3 = CM.tiles_run(CM.p2_marks(run2))
    run, total = CM.counts(empty)
    assert total == 5 * 63 and run == int(run3.sum()) and 0 < run < total
    # with no marks at all the forced set is the floor; conv2's forced tiles on the borders add windows next to them
    floor = CM.tiles_run(np.zeros((1, 100, 100), bool))
    assert (run3 | floor).sum() == run3.sum() and floor.sum() <= run
    for T in (0, 25, 50, 6, 12, 18, 24, 62):                                     # column 0, row-pair crossings, the half tile
        assert floor[0, :, T].all(), T
    assert floor[0, 0, :7].all() and floor[0, 4, 57:].all()                      # first / last row pair of the image
    assert not floor[0, 1, 1] and not floor[0, 2, 30]


def test_a_window_edge_decides():
    """one marked p2 pixel runs exactly the tiles whose 4 x 18 window holds it (beyond the forced ones)."""
    floor = CM.tiles_run(np.zeros((1, 100, 100), bool))[0]
    for (y, x) in ((20, 40), (19, 16), (21, 17), (39, 15), (40, 50), (50, 33)):
        m = np.zeros((1, 100, 100), bool)
        m[0, y, x] = True
        got = CM.tiles_run(m)[0] & ~floor
        want = np.zeros_like(got)
        for step in range(5):
            for T in range(63):
                rp, x0 = divmod(16 * T, 100)
                r0 = 20 * step - 1 + 2 * rp
                want[step, T] = (r0 <= y <= r0 + 3) and (x0 - 1 <= x <= x0 + 16)
        assert np.array_equal(got, want & ~floor), (y, x)
        assert got.any()


def test_scenes_leave_room_on_both_sides():
    run, total = CM.counts(np.zeros((1, TM.SIDE, TM.SIDE), bool))
    assert 0 < run < total
    rs = np.random.RandomState(3)
    brawl = _discs([(360 + rs.randint(0, 40), rs.randint(0, 40)) for _ in range(8)]
                   + [(300 + rs.randint(0, 100), rs.randint(0, 100)) for _ in range(20)], radius=4)
    run, total = CM.counts(brawl)
    assert 0.2 * total < run < total, (run, total)
