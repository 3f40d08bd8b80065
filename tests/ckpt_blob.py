"""numpy restatement of the replay-memory checkpoint blob (TEST ONLY), written from the layout text in include/ofx.h
("checkpoint: export / import of the replay memory"), not from the C: encode(dict) -> bytes, decode(bytes) -> dict.

The dict: scalars W, H, M, C, F, n, per, alpha, eps; the raw arrays under their header names (frame_tick [n][F],
frame_head, cur_slot, head, count [n], appended int64 [n], rows TRANSITION [n][C], has_prev, latched uint8 [n][M],
prev_iaction / prev_px / prev_py / prev_tick / prev_slot int32 [n][M], prev_head float32 [n][M][8], and with per
mass float32 [n][C], mmax float32 [n]); and `maps` uint32 [n][F][2][W*H/32], the frame ring unpacked."""
import struct

import numpy as np

MAGIC, VERSION, HEADER = 0x5258464F, 1, 80
TRANSITION = np.dtype([("tick_prev", "<i4"), ("tick_next", "<i4"), ("frame_prev", "<i4"), ("frame_next", "<i4"),
                       ("ship", "<i4"), ("iaction", "<i4"), ("px", "<i4"), ("py", "<i4"), ("reward", "<i4"), ("done", "<i4"),
                       ("head_prev", "<f4", 8), ("head_next", "<f4", 8)])
assert TRANSITION.itemsize == 104


def raw_arrays(d):
    """(name, dtype, shape) of the raw section's arrays, in order."""
    n, M, C, F = d["n"], d["M"], d["C"], d["F"]
    out = [("frame_tick", "<i4", (n, F)), ("frame_head", "<i4", (n,)), ("cur_slot", "<i4", (n,)), ("rows", TRANSITION, (n, C)),
           ("head", "<i4", (n,)), ("count", "<i4", (n,)), ("appended", "<i8", (n,)), ("has_prev", "u1", (n, M)),
           ("latched", "u1", (n, M))]
    out += [(k, "<i4", (n, M)) for k in ("prev_iaction", "prev_px", "prev_py", "prev_tick", "prev_slot")]
    out += [("prev_head", "<f4", (n, M, 8))]
    if d["per"]:
        out += [("mass", "<f4", (n, C)), ("mmax", "<f4", (n,))]
    return out


def layout(d):
    """name -> (offset in the blob, bytes without padding) of every raw array, plus the section starts `raw`, `counts`,
    `pairs` (-> offset) for a dict or a decoded header."""
    at, out = HEADER, {"raw": HEADER}
    for name, dt, shape in raw_arrays(d):
        nb = int(np.dtype(dt).itemsize * np.prod(shape, dtype=np.int64))
        out[name] = (at, nb)
        at += (nb + 7) // 8 * 8
    out["counts"] = at
    out["pairs"] = at + 4 * d["n"] * d["F"] * 2
    return out


def encode(d):
    words = d["W"] * d["H"] // 32
    maps = np.ascontiguousarray(d["maps"], "<u4").reshape(d["n"] * d["F"] * 2, words)
    raw = b""
    for name, dt, shape in raw_arrays(d):
        a = np.ascontiguousarray(d[name], dt)
        assert a.shape == shape, (name, a.shape, shape)
        b = a.tobytes()
        raw += b + b"\0" * (-len(b) % 8)
    counts = np.count_nonzero(maps, axis=1).astype("<u4")
    at = np.flatnonzero(maps)                        # row-major: map order, ascending word index inside a map
    pairs = np.empty((len(at), 2), "<u4")
    pairs[:, 0], pairs[:, 1] = at % words, maps.reshape(-1)[at]
    head = struct.pack("<II8i2f4Q", MAGIC, VERSION, d["W"], d["H"], d["M"], d["C"], d["F"], words, d["n"], int(d["per"]),
                       d["alpha"] if d["per"] else 0.0, d["eps"] if d["per"] else 0.0, len(raw), counts.nbytes, pairs.nbytes, 0)
    assert len(head) == HEADER
    return head + raw + counts.tobytes() + pairs.tobytes()


def header(blob):
    b = bytes(memoryview(np.ascontiguousarray(blob))[:HEADER]) if not isinstance(blob, bytes) else blob[:HEADER]
    v = struct.unpack("<II8i2f4Q", b)
    assert v[0] == MAGIC and v[1] == VERSION
    d = dict(zip(("W", "H", "M", "C", "F", "words", "n", "per", "alpha", "eps", "raw_bytes", "count_bytes", "pair_bytes"), v[2:]))
    return d


SCALARS = ("W", "H", "M", "C", "F", "per", "alpha", "eps")


def concat(dicts):
    """The decoded dicts of consecutive chunks of one memory -> the dict of the chunk that spans them: every raw array,
    `maps` and (where the dicts carry them) `counts` concatenated along n; the scalars must agree."""
    dicts = list(dicts)
    first = dicts[0]
    out = {k: first[k] for k in SCALARS}
    for d in dicts[1:]:
        for k in SCALARS:
            same = np.float32(d[k]) == np.float32(first[k]) if k in ("alpha", "eps") else d[k] == first[k]
            assert same, (k, d[k], first[k])
    out["n"] = int(sum(d["n"] for d in dicts))
    names = [name for name, _, _ in raw_arrays(first)] + ["maps"] + (["counts"] if all("counts" in d for d in dicts) else [])
    for name in names:
        for d in dicts:
            assert len(d[name]) == d["n"], name
        out[name] = np.concatenate([d[name] for d in dicts], axis=0)
    return out


def decode(blob):
    buf = (np.ascontiguousarray(blob).view(np.uint8).reshape(-1) if isinstance(blob, np.ndarray)
           else np.frombuffer(bytes(blob), np.uint8))
    d = header(buf[:HEADER].tobytes())
    words = d["words"]
    assert words == d["W"] * d["H"] // 32
    lay = layout(d)
    for name, dt, shape in raw_arrays(d):
        at, nb = lay[name]
        d[name] = buf[at:at + nb].view(dt).reshape(shape).copy()
    n_maps = d["n"] * d["F"] * 2
    assert lay["counts"] == HEADER + d["raw_bytes"] and d["count_bytes"] == 4 * n_maps
    counts = buf[lay["counts"]:lay["pairs"]].view("<u4")
    assert d["pair_bytes"] == 8 * int(counts.sum()) and len(buf) == lay["pairs"] + d["pair_bytes"]
    pairs = buf[lay["pairs"]:].view("<u4").reshape(-1, 2)
    maps = np.zeros((n_maps, words), np.uint32)
    maps.reshape(-1)[np.repeat(np.arange(n_maps, dtype=np.int64) * words, counts) + pairs[:, 0]] = pairs[:, 1]
    d["counts"] = counts.reshape(d["n"], d["F"], 2).copy()
    d["maps"] = maps.reshape(d["n"], d["F"], 2, words)
    return d
