"""The host-side builders of tests/test_gpu_forward_obs.py (tests/obs_batches.py), checked without a GPU: a wrong
builder would make the GPU comparisons run on other maps than they claim."""
import numpy as np
import pytest

from tests import obs_batches as OB


@pytest.mark.parametrize("name", OB.PATTERNS)
def test_patterns_round_trip_through_unpackbits(name):
    x = OB.pattern_maps(name, 2, np.random.RandomState(3))
    bits = OB.pack_maps(x)
    assert bits.dtype == np.uint32 and bits.shape == (2, 2, OB.WORDS)
    back = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(2, 2, 400, 400)
    assert np.array_equal(back, x.astype(np.uint8))
    assert np.array_equal(OB.unpack_maps(bits), back)
    # what every pattern is meant to be
    share = x.reshape(2, 2, -1).mean(axis=-1)
    want = {"zero": ((0, 0), (0, 0)), "ones": ((1, 1), (1, 1)), "dense": ((0.29, 0.31), (0.045, 0.055)),
            "half": ((0.145, 0.155), (0.009, 0.011)), "frame": ((1596 / 160000,) * 2,) * 2,
            "ship_only": ((0.29, 0.31), (0, 0)), "laser_only": ((0, 0), (0.29, 0.31))}[name]
    for plane in (0, 1):
        assert (want[plane][0] <= share[:, plane]).all() and (share[:, plane] <= want[plane][1]).all(), (name, share)
    if name == "half":
        assert not x[:, 0, :, 200:].any() and not x[:, 1, :200, :].any()
    if name == "frame":
        assert not x[:, :, 1:399, 1:399].any() and x[:, :, 0].all() and x[:, :, :, 399].all()
    if name in ("dense", "half", "ship_only", "laser_only"):
        assert not np.array_equal(x[0], x[1])          # the random patterns differ between observations


def test_layout_is_the_one_the_gather_documents():
    """[n][2][W*H/32]: observation-major, ship map then laser map, pixel p = y * 400 + x as bit p & 7 of byte p >> 3."""
    x = np.zeros((3, 2, 400, 400), bool)
    pix = [(0, 0, 0, 0), (0, 1, 0, 1), (1, 0, 7, 8), (2, 1, 399, 399), (2, 0, 123, 31), (1, 1, 200, 32)]   # n, plane, y, x
    for n, plane, y, xx in pix:
        x[n, plane, y, xx] = True
    raw = OB.pack_maps(x).reshape(-1).view(np.uint8)
    assert raw.size == 3 * 2 * 20000
    want = np.zeros_like(raw)
    for n, plane, y, xx in pix:
        p = y * 400 + xx
        want[(n * 2 + plane) * 20000 + (p >> 3)] |= 1 << (p & 7)
    assert np.array_equal(raw, want)
    # the same bit seen as the uint32 word the kernels load: word p >> 5, bit p & 31
    words = OB.pack_maps(x)
    for n, plane, y, xx in pix:
        p = y * 400 + xx
        assert (int(words[n, plane, p >> 5]) >> (p & 31)) & 1


def test_sweep_batch_hits_every_row_and_column_once_per_map():
    bits = OB.sweep_bits()
    assert bits.shape == (400, 2, OB.WORDS) and bits.dtype == np.uint32
    x = OB.unpack_maps(bits)
    assert (x.reshape(400, 2, -1).sum(axis=-1) == 1).all()              # one bit per map and observation
    for plane in (0, 1):
        ys, xs = [], []
        for k in range(400):
            (y, xx), = np.argwhere(x[k, plane])
            assert (int(y), int(xx)) == OB.sweep_pixels(k)[plane]
            ys.append(int(y)); xs.append(int(xx))
        assert sorted(ys) == list(range(400)) and sorted(xs) == list(range(400))


def test_frame_probes_are_where_they_say():
    corners, edges, near = OB.frame_probes()
    on_frame = lambda p: p[0] in (0, 399) or p[1] in (0, 399)
    assert len(set(corners)) == 4 and all(p[0] in (0, 399) and p[1] in (0, 399) for p in corners)
    assert len(set(edges)) == 8 and all(on_frame(p) and p not in corners for p in edges)
    assert {(p[1] == 0, p[1] == 399, p[0] == 0, p[0] == 399).index(True) for p in edges} == {0, 1, 2, 3}   # all four edges
    assert near == [(1, 1), (398, 398)]
