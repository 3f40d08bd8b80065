"""The CPU model of the sparse streaming trunk (tests/trunk_sparse_model.py) against its own definitions: the lane map of
the table phase takes every (row, pair) of a step exactly once, and the run set of the GEMM phase holds every M-tile
whose window sees a set bit."""
import numpy as np
import pytest

from tests import trunk_sparse_model as TM


@pytest.mark.parametrize("step", [0, 7, 19])       # 11, 10 and 9 new rows
def test_lane_map_is_a_bijection(step):
    pa, pb = TM.step_rows(step)
    nrow = pb - pa
    assert nrow == {0: 11, 7: 10, 19: 9}[step]
    seen = np.zeros((nrow, TM.PAIRS), int)
    for npass in range(2 if nrow > TM.TH else 1):
        py, pp, valid = TM.lane_map(nrow, npass)
        assert ((0 <= py[valid]) & (py[valid] < nrow) & (0 <= pp[valid]) & (pp[valid] < TM.PAIRS)).all()
        np.add.at(seen, (py[valid], pp[valid]), 1)
    assert (seen == 1).all()
    if nrow <= TM.TH:                              # one pass of the 16 waves
        assert TM.lane_map(nrow, 0)[2].sum() == nrow * TM.PAIRS


def test_step_rows_cover_the_image_once():
    rows = np.concatenate([np.arange(*TM.step_rows(s)) for s in range(TM.STEPS)])
    assert np.array_equal(rows, np.arange(TM.P1))


def _discs(rs, n, ships, lasers):
    bits = np.zeros((n, TM.SIDE, TM.SIDE), bool)
    yy, xx = np.mgrid[:TM.SIDE, :TM.SIDE]
    for g in range(n):
        for r, k in ((8, ships), (1, lasers)):
            for cy, cx in rs.randint(0, TM.SIDE + 1, (k, 2)):
                bits[g] |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return bits


@pytest.mark.parametrize("seed,ships,lasers", [(1, 8, 60), (2, 1, 10), (3, 0, 1), (4, 0, 0)])
def test_run_set_holds_every_tile_that_sees_a_bit(seed, ships, lasers):
    """Brute force from the definition of the network: output pixel (Y2, X2) of conv2 + pool reads p1 rows 2 Y2 - 1 ..
    2 Y2 + 2 x columns 2 X2 - 1 .. 2 X2 + 2, and p1 pixel (Y, X) reads image rows 2 Y - 1 .. 2 Y + 2 x columns
    2 X - 1 .. 2 X + 2.  A tile owning an output pixel whose p1 window is not all-constant must run."""
    rs = np.random.RandomState(seed)
    bits = _discs(rs, 3, ships, lasers)
    marks = TM.pair_marks(bits)
    pad = np.pad(bits, ((0, 0), (1, 2), (1, 2)))
    p1 = np.zeros((3, TM.P1, TM.P1), bool)                                      # p1 pixel differs from the constant
    for dr in range(4):
        for dc in range(4):
            p1 |= pad[:, dr:dr + TM.SIDE:2, dc:dc + TM.SIDE:2]
    assert not (p1 & ~np.repeat(marks, 2, axis=2)).any()                        # a pair's mark covers both of its pixels
    pad1 = np.pad(p1, ((0, 0), (1, 2), (1, 2)))
    need = np.zeros((3, TM.P1 // 2, TM.P1 // 2), bool)                          # pooled conv2 output pixel is not constant
    for dr in range(4):
        for dc in range(4):
            need |= pad1[:, dr:dr + TM.P1:2, dc:dc + TM.P1:2]
    # output pixel (Y2, X2) <- conv2 pixels of row pair Y2, columns 2 X2, 2 X2 + 1 <- tile (step Y2 // 5, (200 (Y2 % 5) + 2 X2) // 16)
    Y2, X2 = np.mgrid[:TM.P1 // 2, :TM.P1 // 2]
    step, T = Y2 // 5, (TM.P1 * (Y2 % 5) + 2 * X2) // 16
    run = TM.tiles_run(marks)
    assert run.shape == (3, TM.STEPS, TM.NT)
    assert not (need & ~run[:, step, T]).any()
    if ships == lasers == 0:
        # the forced floor of an empty image: per step the tiles at 0, 192, 384, 400, 592, 784, 800, 992 (column 0 or a
        # row-pair crossing), and the other 11 tiles of the first and of the last row pair of the image
        assert run.sum() == 3 * (20 * 8 + 2 * 11)
    r, t = TM.table_passes(marks)
    assert 0 <= r <= t == 3 * 321 and (r == 0) == (not marks.any())


def test_unpack_is_packbits_order():
    rs = np.random.RandomState(0)
    a, b = rs.rand(2, TM.SIDE, TM.SIDE) < 0.01, rs.rand(2, TM.SIDE, TM.SIDE) < 0.01
    got = TM.unpack(np.packbits(a.reshape(2, -1), axis=1), np.packbits(b.reshape(2, -1), axis=1))
    assert np.array_equal(got, a | b)
