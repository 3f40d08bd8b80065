"""CPU restatement of the symmetry-augmentation contract in include/ofx.h (ofx_obs_transform, ofx_replay_augment): the
eight isometries of the square on 1-bit maps, observation heads and pointers, their inverse and composition tables, and
the Philox draw of one element per row.  Everything here is exact: integer index arithmetic, and float32 subtractions of
integer values."""
import numpy as np

from oracle.pyoracle import philox

SYM_TRANSPOSE, SYM_FLIP_X, SYM_FLIP_Y = 1, 2, 4      # applied in this order to a position (x, y)
STREAM_AUGMENT = 8


def apply_xy(g, x, y, W, H):
    """Element g on a position; x, y numbers or arrays of one type (int32 pointers, float32 head elements)."""
    if g & SYM_TRANSPOSE:
        x, y = y, x
    if g & SYM_FLIP_X:
        x = type(x)(W - 1) - x if np.isscalar(x) else np.asarray(W - 1, x.dtype) - x
    if g & SYM_FLIP_Y:
        y = type(y)(H - 1) - y if np.isscalar(y) else np.asarray(H - 1, y.dtype) - y
    return x, y


def _tables():
    """Inverse and composition of the eight elements, from their action on three points of a square that no two
    elements move alike.  COMPOSE[a][b] is the one element that does `a first, then b`."""
    W = H = 7
    pts = [(0, 0), (1, 0), (2, 5)]
    act = lambda g, ps: tuple(apply_xy(g, x, y, W, H) for x, y in ps)
    image = {act(g, pts): g for g in range(8)}
    assert len(image) == 8
    compose = [[image[act(b, act(a, pts))] for b in range(8)] for a in range(8)]
    inverse = [compose[a].index(0) for a in range(8)]
    return inverse, compose


INVERSE, COMPOSE = _tables()


def unpack_map(words, W, H):
    """uint32 [W*H/32] (pixel p = y*W + x at bit p & 31 of word p >> 5) -> uint8 [H][W]."""
    return np.unpackbits(np.ascontiguousarray(words, "<u4").view(np.uint8), bitorder="little").reshape(H, W)


def pack_map(m):
    return np.packbits(np.ascontiguousarray(m, np.uint8).reshape(-1), bitorder="little").view("<u4")


def transform_image(g, m):
    """out[y'][x'] = in[y][x] for an [H][W] image."""
    if g & SYM_TRANSPOSE:
        m = m.T
    if g & SYM_FLIP_X:
        m = m[:, ::-1]
    if g & SYM_FLIP_Y:
        m = m[::-1]
    return m


def transform_maps(g, bits, W, H):
    """bits uint32 [2][W*H/32] of one observation -> the same shape under element g (g > 7: unchanged)."""
    if g > 7:
        return np.array(bits, np.uint32)
    return np.stack([pack_map(transform_image(g, unpack_map(b, W, H))) for b in bits]).astype(np.uint32)


def transform_head(g, vec8, W, H):
    """float32 [8]: elements (2, 3) and (6, 7) are positions, the others keep their bits."""
    out = np.array(vec8, np.float32)
    if g > 7:
        return out
    for k in (2, 6):
        out[k], out[k + 1] = apply_xy(g, np.float32(out[k]), np.float32(out[k + 1]), W, H)
    return out


def transform_pointer(g, ptr, W, H):
    out = np.array(ptr, np.int32)
    if g <= 7:
        out[0], out[1] = apply_xy(g, np.int32(out[0]), np.int32(out[1]), W, H)
    return out


def draw_ops(seed, draw, first, n, op_mask, arena_base=0, ships=None):
    """The element of rows first .. first + n - 1 of one draw: the ofx_draw_int(rr[0], k - 1)-th set bit of the mask in
    ascending order, rr = Philox counter (arena_base, first + d, draw, stream 8); 0 for a padding row (ship < 0)."""
    allowed = [g for g in range(8) if op_mask >> g & 1]
    out = np.zeros(n, np.uint8)
    for d in range(n):
        if ships is not None and ships[d] < 0:
            continue
        r = philox(arena_base, first + d, draw, STREAM_AUGMENT, seed)
        out[d] = allowed[(int(r[0]) * len(allowed)) >> 32]
    return out


def augment_rows(ops, rows, bits_prev, bits_next, W, H):
    """ofx_replay_augment's effect on a gathered batch (structured rows [n], maps uint32 [n][2][words]) -> copies."""
    rows, bits_prev, bits_next = rows.copy(), np.array(bits_prev, np.uint32), np.array(bits_next, np.uint32)
    for d, g in enumerate(ops):
        g = int(g)
        if rows["ship"][d] < 0 or g == 0:
            continue
        bits_prev[d], bits_next[d] = transform_maps(g, bits_prev[d], W, H), transform_maps(g, bits_next[d], W, H)
        rows["head_prev"][d] = transform_head(g, rows["head_prev"][d], W, H)
        rows["head_next"][d] = transform_head(g, rows["head_next"][d], W, H)
        rows["px"][d], rows["py"][d] = transform_pointer(g, (rows["px"][d], rows["py"][d]), W, H)
    return rows, bits_prev, bits_next
