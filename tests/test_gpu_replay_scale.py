"""The replay memory at the sizes the trainer runs it at (ofx_replay.hip): exports and imports of chunks of more than one
scan segment (launch_pack_scan: PACK_SEG = 2048 counts per segment, more than 1024 segments), k_replay_scan and
k_replay_level_mmax over more than 1024 arenas, and the global sampler's group chain over more than two groups.

Part 1's reference is the single-segment export, which tests/test_gpu_checkpoint.py holds to the host inspections: the
same arenas exported in pieces of at most 2048 maps, decoded, stitched (tests/ckpt_blob.py: concat) and encoded.  Part
2's references are the restatements tests/per_oracle.py and tests/global_sample_oracle.py, oracle.pyoracle.replay_sample
and the host inspections.  Every comparison is exact but the importance-sampling weights (rtol 1e-6, as in
tests/test_global_sampler.py and tests/test_prioritized_replay.py).

One precondition of part 1 cannot hold at the frame counts of the cases "400" (F = 32) and "many" (F = 256): a segment
boundary strictly inside an arena's frame ring.  An arena has 2 F maps, 2 F divides 2048 for both, so every boundary
falls between two arenas.  The case "odd" (F = 22, 44 maps per arena) is there for that boundary."""
import numpy as np
import pytest

from tests import ckpt_blob
from tests import global_sample_oracle as gso
from tests import per_oracle
from tests import replay_cases as rc
from tests.train_state import check_decoded, inspect_replay

pytestmark = pytest.mark.gpu

SEG = 2048                                   # PACK_SEG
SEED = 0x0F160061
BETA = 0.4


# ================================================================== 1. chunks of more than one scan segment
def _masks_100(t):
    """100 arenas x 4 ships: arenas 32 .. 66 never capture (a whole segment of the chunks (0, 100) and (3, 97) stays
    empty), arenas 5, 31, 67 and 98 stop after lock-step 9 (their later slots stay empty: with arena 31 a run of empty
    slots crosses the boundary to arena 32), arena 2 captures with one ship."""
    mk = np.ones((100, 4), np.uint8)
    mk[32:67] = 0
    mk[[5, 31, 67, 98]] = t < 10
    mk[2, 1:] = 0
    return mk


def _masks_many(t, N=4101):
    """4101 arenas x 2 ships: arenas 8 .. 15 (segments 2 and 3 of the whole memory) and every 97th never capture, every
    7th stops after lock-step 39."""
    a = np.arange(N)
    on = ~(((a >= 8) & (a < 16)) | (a % 97 == 5)) & ((a % 7 != 3) | (t < 40))
    return np.repeat(on.astype(np.uint8)[:, None], 2, 1)


def _corners(b):
    """Ship 0 at (0, 0) and ship 1 at (W - 1, H - 1) in arenas 0, 3 and the last: the first and the last word of a map."""
    from ofighters_amd import _native as nat
    x, y = b.get(nat.F_SHIP_X).copy(), b.get(nat.F_SHIP_Y).copy()
    for a in (0, 3, b.N - 1):
        x[a, 0] = y[a, 0] = 0
        x[a, 1], y[a, 1] = b.W - 1, b.H - 1
    b.set_ships(x=x, y=y)


# chunks: (arena0, n) -> segments; piece: arenas per single-segment export; some: what at least one chunk must show
CASES = {
    "400": dict(N=100, M=4, capacity=24, frames=32, ticks=45, restart_every=23, masks=_masks_100, width=400, height=400,
                after_spawn=_corners, piece=32, chunks={(0, 32): 1, (0, 33): 2, (3, 97): 4, (0, 100): 4},
                some=("empty run across a boundary", "zero segment between nonzero ones")),
    "odd": dict(N=100, M=4, capacity=12, frames=22, ticks=30, restart_every=16, masks=_masks_100, width=64, height=64,
                after_spawn=_corners, piece=46, chunks={(0, 100): 3, (1, 98): 3},
                some=("boundary inside a frame ring", "empty run across a boundary")),
    "many": dict(N=4101, M=2, capacity=8, frames=256, ticks=300, restart_every=12, masks=_masks_many, width=32, height=32,
                 ship_radius=2, laser_radius=1, pool_pairs=256 * 64, piece=4, chunks={(0, 4101): 1026},
                 some=("empty run across a boundary", "zero segment between nonzero ones")),
}
_BUILD = ("N", "M", "capacity", "frames", "ticks", "restart_every", "masks", "width", "height", "ship_radius", "laser_radius",
          "pool_pairs", "after_spawn")


class _Memory:
    """A case's memory on one handle, its single-segment exports and its big exports, each made once."""

    def __init__(self, case, packed):
        self.c = c = CASES[case]
        self.packed = packed
        kw = {k: c[k] for k in _BUILD if k in c}
        if not packed:
            kw.pop("pool_pairs", None)
        self.b = rc.rollout(alpha=0.6, packed=packed, seed=SEED, **kw)
        rc.spread_masses(self.b, 7)
        self._piece, self._big, self._ref = {}, {}, {}

    def fresh(self):
        """An empty handle of the same build."""
        from ofighters_amd import ArenaBatch
        c = self.c
        cfg = {k: c[k] for k in ("width", "height", "ship_radius", "laser_radius") if k in c}
        b = ArenaBatch(c["N"], c["M"], **cfg)
        b.replay_create(c["capacity"], c["frames"], packed=self.packed, pool_pairs=c.get("pool_pairs", 0) if self.packed else 0)
        b.replay_prioritize(0.6, 1e-3)
        b.spawn_random(SEED)
        return b

    def pieces(self, a0, n):
        """[((arena0, n), blob)] covering [a0, a0 + n) in exports of at most one segment each."""
        out = []
        for p0 in range(a0, a0 + n, self.c["piece"]):
            key = (p0, min(self.c["piece"], a0 + n - p0))
            assert 2 * self.b.replay_frames * key[1] <= SEG
            if key not in self._piece:
                self._piece[key] = self.b.replay_export(*key)
            out.append((key, self._piece[key]))
        return out

    def big(self, a0, n):
        if (a0, n) not in self._big:
            self._big[(a0, n)] = self.b.replay_export(a0, n)
        return self._big[(a0, n)]


    def reference(self, a0, n):
        """(dict, blob) of the chunk stitched from its single-segment exports: decoded, concatenated, encoded."""
        if (a0, n) not in self._ref:
            d = ckpt_blob.concat([ckpt_blob.decode(blob) for _, blob in self.pieces(a0, n)])
            self._ref[(a0, n)] = (d, np.frombuffer(ckpt_blob.encode(d), np.uint8))
        return self._ref[(a0, n)]


@pytest.fixture(scope="module", params=[(case, packed) for case in CASES for packed in (False, True)],
                ids=lambda p: "%s-%s" % (p[0], "packed" if p[1] else "dense"))
def memory(request):
    """The case's memory and, computed once for the tests that share it, the reference of every chunk.  Measured on the
    MI355X machine (profiles/r26_replay_scale.txt): this set-up takes 0.83 s (dense) and 0.78 s (packed) for the case
    "many" - 1026 single-segment exports (0.41 s) and their decode, concat and encode over 2 099 712 maps (0.39 s) -,
    above the 0.61 s of the slowest test of tests/test_global_sampler.py in the same run; every test's own call stays
    below it (0.56 s at the most).  With 100 lock-steps in place of 300 it still takes 0.73 s: the cost follows the
    segment count, which is the point of the case."""
    m = _Memory(*request.param)
    m.case = request.param[0]
    for a0, n in m.c["chunks"]:
        m.reference(a0, n)
    yield m
    m.b.close()


def _preconditions(d, label):
    """What the stitched reference of a chunk shows the segmented scan; printed, the caller asserts."""
    F, n_maps = d["F"], d["n"] * d["F"] * 2
    counts = d["counts"].reshape(-1).astype(np.int64)
    bounds = np.arange(SEG, n_maps, SEG)                                   # the first map of segments 1 ..
    seg = np.add.reduceat(counts, np.arange(0, n_maps, SEG))
    empty = np.repeat(d["frame_tick"].reshape(-1) < 0, 2)
    nz = seg > 0
    pre = {
        "segments": len(seg),
        "last segment": n_maps - SEG * (len(seg) - 1),
        "boundary inside a frame ring": bool((bounds % (2 * F) != 0).any()),
        "empty run across a boundary": bool((empty[bounds - 1] & empty[bounds]).any()),
        "zero segment between nonzero ones": any(not nz[k] and nz[:k].any() and nz[k + 1:].any() for k in range(len(seg))),
        "first word set": bool((d["maps"][..., 0] != 0).any()),
        "last word set": bool((d["maps"][..., -1] != 0).any()),
        "neighbouring segments differ": bool((np.diff(seg) != 0).any()),
        "zero segments": int((~nz).sum()), "pairs": int(counts.sum()), "largest segment": int(seg.max()),
        "live slots": int((~empty).sum()) // 2, "slots": n_maps // 2,
    }
    print("replay-scale %s: %s" % (label, pre))
    return pre


def test_export_of_many_segments_is_the_stitched_single_segment_exports(memory):
    m = memory
    b, c, case, packed = m.b, m.c, m.case, m.packed
    cnt, app = b.replay_count()
    print("replay-scale %s-%s: rows %d, arenas without rows %d, with a wrapped row ring %d" % (
        case, "packed" if packed else "dense", cnt.sum(), (cnt == 0).sum(), (app > c["capacity"]).sum()))
    assert (cnt == 0).any() and (app > c["capacity"]).any()
    if case == "400":
        sample = sorted({0, 2, 3, 5, 31, 32, 33, 34, 35, 63, 64, 66, 67, 95, 96, 98, 99})
        ins = inspect_replay(b, c["ticks"], arenas=sample)
    seen = set()
    for (a0, n), n_seg in c["chunks"].items():
        label = "%s-%s (%d, %d)" % (case, "packed" if packed else "dense", a0, n)
        ref_d, ref = m.reference(a0, n)
        pre = _preconditions(ref_d, label)
        assert pre["segments"] == n_seg == -(-2 * n * b.replay_frames // SEG)
        assert pre["first word set"] and pre["last word set"]
        assert n_seg == 1 or pre["neighbouring segments differ"]
        seen |= {k for k in c["some"] if pre[k]}
        ft = ref_d["frame_tick"]
        assert ((ft < 0).any(axis=1) & (ft >= 0).any(axis=1)).any()       # an arena that stopped early: a partly empty ring
        if case == "many":
            assert 2 * pre["live slots"] > pre["slots"]                    # most slots are filled
        else:
            assert (ft >= 0).all(axis=1).any()                             # a ring that wrapped
        big = m.big(a0, n)
        print("replay-scale %s: blob %d bytes" % (label, big.nbytes))
        assert big.nbytes < 256 << 20
        assert big.nbytes == ref.nbytes and np.array_equal(big, ref)
        assert b.replay_export_bytes(a0, n) == big.nbytes
        assert np.array_equal(b.replay_export(a0, n), big)                 # byte-identical again
        if case == "400":
            inside = [a for a in sample if a0 <= a < a0 + n]
            firsts = [a0 + k * c["piece"] for k in range(1, n_seg)]
            assert all(f - 1 in inside and f in inside for f in firsts)    # both sides of every boundary in the chunk
            check_decoded(ckpt_blob.decode(big), ins, a0, only=inside)
    assert seen == set(c["some"]), (seen, c["some"])


def test_import_of_many_segments_round_trips(memory):
    """The big blob into a fresh handle of the same build; that handle's single-segment exports are the original's."""
    m = memory
    for a0, n in m.c["chunks"]:
        pieces, big = m.pieces(a0, n), m.big(a0, n)
        f = m.fresh()
        f.replay_import(a0, n, big)
        for key, blob in pieces:
            assert np.array_equal(f.replay_export(*key), blob), (a0, n, key)
        f.close()


# ========================================================================== 2. more than 1024 arenas
M2, CAP2, TICKS2, BATCH2, WINDOW = 4, 12, 12, 8, 256
EMPTY2 = (256, 511)                          # besides arena 0: an empty arena at a sampler group's start and at one's end
SCALE = {"1025-0": (1025, 0, 0), "1025-4": (1025, 4, 0), "2500-0": (2500, 0, 0), "2500-4": (2500, 4, 0),
         "2500-0-base4096": (2500, 0, 4096)}


def _group_ends(N):
    """First and last arena of every sampler group but the first (arena 0 is empty)."""
    return sorted({a for k in range(1, -(-N // gso.GROUP)) for a in (k * gso.GROUP, min(N, (k + 1) * gso.GROUP) - 1)}
                  - set(EMPTY2))


def _snapshot(b):
    """Every arena's rows and masses, oldest first ([N][C]; entries from the arena's count on mean nothing), and the
    decoded export of the whole memory they were read from - one export of tens of segments (part 1 holds those to the
    single-segment export) in place of thousands of host inspections."""
    d = ckpt_blob.decode(b.replay_export(0, b.N))
    order = (d["head"][:, None] - d["count"][:, None] + np.arange(d["C"])[None, :]) % d["C"]
    return np.take_along_axis(d["rows"], order, 1), np.take_along_axis(d["mass"], order, 1), d


class _Arenas:
    def __init__(self, case):
        self.case = case
        self.N, self.frames, self.base = N, frames, base = SCALE[case]
        varied = rc.varied_masks(N, M2)

        def masks(t):
            mk = varied(t)
            mk[list(EMPTY2)] = 0
            return np.concatenate([np.zeros((base, M2), np.uint8), mk])
        self.b = b = rc.rollout(N, M2, capacity=CAP2, frames=frames, ticks=TICKS2, seed=SEED, arena_base=base, alpha=1.0,
                                masks=masks, width=64, height=64)
        self.rows, _, d = _snapshot(b)
        self.cnt = cnt = d["count"]
        assert np.array_equal(cnt, b.replay_count()[0])
        assert cnt[0] == 0 and cnt[1] == 1 and 0 < cnt[3] <= 4 < cnt[2] <= 11 and (cnt == CAP2).sum() > N // 2
        assert cnt[list(EMPTY2)].sum() == 0
        # eligibility (tests/packed_ring_model.py: eligible): the oldest rows whose `state` frame left the ring are skipped
        held = np.take_along_axis(d["frame_tick"], np.clip(self.rows["frame_prev"], 0, d["F"] - 1), 1) == self.rows["tick_prev"]
        held &= np.arange(CAP2)[None, :] < cnt[:, None]
        self.skip = np.where(held.any(1), held.argmax(1), cnt).astype(int).tolist()
        self.v = [int(c) - s for c, s in zip(cnt, self.skip)]
        assert (max(self.skip) > 0) == bool(frames), "rows expire exactly when the frame ring is short"
        self.spot = sorted({0, 1, 2, 3, 255, 256, 257, 511, 512, 1023, 1024, N - 1})
        for a in self.spot:                                                # the host inspections agree
            assert self.rows[a, :cnt[a]].tobytes() == b.replay_rows(a).tobytes() and self.skip[a] == rc.stale_rows(b, a), a
        print("replay-scale arenas %s: rows %d eligible %d, scan entries per thread %d, sampler groups %d" % (
            case, cnt.sum(), sum(self.v), -(-N // 1024), -(-N // gso.GROUP)))

    def spread(self):
        """The masses every test starts from (a test that writes masses leaves them for no other): [N][C] oldest first,
        and as the list of every arena's rows' masses."""
        rc.spread_masses(self.b, self.N + self.frames, heavy=_group_ends(self.N))
        _, mass, d = _snapshot(self.b)
        for a in self.spot:
            assert np.array_equal(mass[a, :self.cnt[a]], self.b.replay_priorities(a)), a
        live = np.arange(CAP2)[None, :] < self.cnt[:, None]
        assert mass[live].max() / mass[live].min() > 1e5                   # six decades (alpha = 1)
        return mass, [mass[a, :self.cnt[a]] for a in range(self.N)], d


@pytest.fixture(scope="module", params=list(SCALE))
def arenas(request):
    m = _Arenas(request.param)
    yield m
    m.b.close()


def _per_sample(b, draw):
    slot, n, iw = b.replay_sample_prioritized(SEED, draw, BATCH2, BETA)
    b.sync()
    return (slot.download(np.int32, (b.N, BATCH2)), n.download(np.int32, (b.N,)), iw.download(np.float32, (b.N, BATCH2)),
            (slot, n, iw))


def test_per_arena_samplers_equal_their_restatements_in_every_arena(arenas):
    from oracle import pyoracle
    m = arenas
    b, (_, mass, _) = m.b, m.spread()
    draw = 3
    slot, n = b.replay_sample(SEED, draw, BATCH2)
    b.sync()
    slot, n = slot.download(np.int32, (m.N, BATCH2)), n.download(np.int32, (m.N,))
    pslot, pn, piw, _ = _per_sample(b, draw)
    assert len(set(n.tolist())) > 2 and len(set(pn.tolist())) > 2           # n_sampled varies across the arenas
    want, pwant, wwant = np.full((m.N, BATCH2), -1, np.int32), np.full((m.N, BATCH2), -1, np.int32), np.zeros((m.N, BATCH2), np.float32)
    for a in range(m.N):
        u = pyoracle.replay_sample(m.v[a], BATCH2, SEED, m.base + a, draw)
        want[a, :len(u)] = np.asarray(u, np.int32) + m.skip[a]
        pwant[a], rn, wwant[a] = per_oracle.sample_arena(mass[a], m.skip[a], BATCH2, BETA, SEED, m.base + a, draw)
        assert len(u) == rn == min(BATCH2, m.v[a])
    assert np.array_equal(n, np.minimum(BATCH2, m.v)) and np.array_equal(pn, n)
    assert np.array_equal(slot, want), np.flatnonzero((slot != want).any(1))[:8]
    assert np.array_equal(pslot, pwant), np.flatnonzero((pslot != pwant).any(1))[:8]
    np.testing.assert_allclose(piw, wwant, rtol=1e-6, atol=0)


def _windows(N, off):
    """first entry of the windows of WINDOW rows the issue names, by what they cover."""
    per = -(-N // 1024)                       # arenas per thread of k_replay_scan
    edge = per * (N // (2 * per))             # the first arena of a thread in the middle of the sequence
    total = int(off[N])
    return {"first": 0, "arenas 1023 | 1024": int(off[1024]) - 3, "scan threads' arenas %d | %d" % (edge - 1, edge): int(off[edge]) - 5,
            "last, partial": total - 100, "past the end": total + 7}, edge


def test_windows_of_the_packed_sequence_over_every_arena(arenas):
    """ofx_replay_gather_valid, ofx_replay_window_weights and ofx_replay_update_priorities on windows of the trainer's
    fit_batch rows, placed by the exclusive scan of n_sampled over more than 1024 arenas."""
    from ofighters_amd import DeviceBuffer
    m = arenas
    b, N, case = m.b, m.N, m.case
    before = m.spread()[0]
    slot_h, n_h, iw_h, (slot, n_s, iw) = _per_sample(b, 1)
    off = np.concatenate([[0], np.cumsum(n_h, dtype=np.int64)])
    total = int(off[N])
    ent_a = np.repeat(np.arange(N), n_h)                                   # the packed (arena, j) order
    ent_s = slot_h[np.arange(BATCH2)[None, :] < n_h[:, None]]
    want_rows = m.rows[ent_a, ent_s]
    windows, edge = _windows(N, off)
    rs = np.random.RandomState(N)
    live = np.arange(CAP2)[None, :] < m.cnt[:, None]
    dups = 0
    for name, first in windows.items():
        n_want = min(WINDOW, max(0, total - first))
        arenas_in = ent_a[first:first + n_want]
        print("replay-scale window %s %r: first %d rows %d arenas %s .. %s" % (case, name, first, n_want, arenas_in[:1], arenas_in[-1:]))
        if "1023" in name:
            assert arenas_in[0] <= 1023 and arenas_in[-1] >= 1024
        if "scan" in name:
            assert arenas_in[0] < edge <= arenas_in[-1] and 0 < edge % 1024 and edge % -(-N // 1024) == 0
        rows, got = rc.gather_rows(b, slot, n_s, BATCH2, first, WINDOW)
        b.sync()
        assert got == n_want and {"first": WINDOW, "last, partial": 100, "past the end": 0}.get(name, got) == got
        assert rows.download(b.TRANSITION_DTYPE, (WINDOW,))[:got].tobytes() == want_rows[first:first + got].tobytes()
        out = DeviceBuffer(4 * WINDOW).upload(np.full(WINDOW, 7.0, np.float32))
        b.replay_window_weights_into(iw, n_s, BATCH2, first, WINDOW, out)
        b.sync()
        w = out.download(np.float32, (WINDOW,))
        np.testing.assert_array_equal(w[:got], per_oracle.window_weights(iw_h, n_h, first, WINDOW))
        assert (w[got:] == 7.0).all()                                      # nothing written past the window
        if not got:
            continue
        # ---- the write-back of this window (tests/test_prioritized_replay.py: test_window_weights_and_update)
        td = rs.normal(0, 3, (got, 2)).astype(np.float32)
        assert got >= 4                                                    # the shortest window: 3 rows + the last arena's
        td[got // 4, 0], td[got // 2, 1], td[3 * got // 4, 0] = np.nan, np.inf, -np.inf
        td_d = DeviceBuffer(td.nbytes).upload(td)
        b.replay_update_priorities(slot, n_s, BATCH2, first, got, rows.ptr, td_d.ptr)
        b.sync()
        want = before.astype(np.float64)
        written = np.zeros(before.shape, bool)
        dup = 0
        for d in range(got):                                               # later entries of a duplicated row win
            a, s = ent_a[first + d], ent_s[first + d]
            if np.isfinite(td[d]).all():
                dup += int(written[a, s])
                written[a, s] = True
                want[a, s] = per_oracle.new_mass(td[d, 0], td[d, 1], 1.0, 1e-3)
        assert dup > 0 or got < WINDOW, "no duplicate draw to test the last-write rule"
        dups += dup
        after = _snapshot(b)[1]
        for a in m.spot:
            assert np.array_equal(after[a, :m.cnt[a]], b.replay_priorities(a)), a
        same = live & ~written                                             # every other row of every arena: bit-identical
        assert np.array_equal(after[same], before[same]), (name, np.flatnonzero((after != before) & same)[:8])
        ulp = np.spacing(want[written].astype(np.float32)).astype(np.float64)
        assert (np.abs(after[written] - want[written]) <= 2 * ulp).all(), name
        before = after
    assert dups > 0


def _global(b, draw, n_rows, per):
    arena, slot, w, n, R = b.replay_sample_global(SEED, draw, n_rows, per, BETA if per else 0.0)
    b.sync()
    return (arena.download(np.int32, (n_rows,)), slot.download(np.int32, (n_rows,)),
            w.download(np.float32, (n_rows,)) if per else None, n, R)


def _group_precondition(N, drawn, label):
    """The drawn arenas hold the first and the last arena of at least three groups, and an empty arena sits at a group's
    start or end."""
    groups = [k for k in range(-(-N // gso.GROUP))
              if k * gso.GROUP in drawn and min(N, (k + 1) * gso.GROUP) - 1 in drawn]
    print("replay-scale global %s: %d arenas drawn, first and last arena drawn of groups %s" % (label, len(drawn), groups))
    assert len(groups) >= 3 and EMPTY2[0] % gso.GROUP == 0 and EMPTY2[1] % gso.GROUP == gso.GROUP - 1


def test_global_sampler_equals_restatement_over_many_groups(arenas):
    m = arenas
    b, N, case = m.b, m.N, m.case
    mass = m.spread()[1]
    R = sum(m.v)
    assert N > 2 * gso.GROUP and R > 4096 and m.v[EMPTY2[0]] == m.v[EMPTY2[1]] == 0
    for n_rows in (1, 257, 4096, R, R + 5):
        arena, slot, _, n, gotR = _global(b, 0, n_rows, False)
        ra, rs_, rn, rR = gso.sample_uniform(m.v, m.skip, n_rows, SEED, m.base, 0)
        assert (n, gotR) == (rn, rR) == (min(n_rows, R), R)
        assert np.array_equal(arena[:n], ra) and np.array_equal(slot[:n], rs_), n_rows
        assert (arena[n:] == -1).all() and (slot[n:] == -1).all()
        assert (np.diff(arena[:n].astype(np.int64) * 2 ** 20 + slot[:n]) > 0).all()      # strictly ascending: no row twice
        if n_rows == R:
            _group_precondition(N, set(arena[:n].tolist()), case + " uniform")
    drawn = set()
    for n_rows in (1, 257, 4096):
        for d in (0, 1):
            arena, slot, w, n, gotR = _global(b, d, n_rows, True)
            ra, rs_, rw, rn, rR = gso.sample_prioritized(mass, m.skip, n_rows, BETA, SEED, m.base, d)
            assert (n, gotR) == (rn, rR) == (n_rows, R)
            assert np.array_equal(arena, ra) and np.array_equal(slot, rs_), (n_rows, d)
            np.testing.assert_allclose(w, rw, rtol=1e-6, atol=0, err_msg="n_rows %d draw %d" % (n_rows, d))
            assert (np.diff(arena.astype(np.int64) * 2 ** 20 + slot) >= 0).all()
            drawn |= set(arena.tolist())
    _group_precondition(N, drawn, case + " prioritized")


def _table(arena, slot, N):
    """The slot[N][batch] / n_sampled[N] table whose packed (arena, j) order is the sorted list."""
    per = np.bincount(arena, minlength=N)
    tab = np.full((N, int(per.max())), -1, np.int32)
    fill = np.zeros(N, int)
    for a, s in zip(arena, slot):
        tab[a, fill[a]] = s
        fill[a] += 1
    return tab, per.astype(np.int32), int(per.max())


def test_list_gather_and_levelled_write_back_over_every_arena(arenas):
    """The sampled (arena, slot) list: its gather is the window gather's rows, its write-back lands as
    gso.write_back says, and every arena's running maximum becomes the global one (k_replay_level_mmax over more than
    1024 arenas) - read from the export of the whole memory, itself one of many segments."""
    from ofighters_amd import DeviceBuffer
    m = arenas
    b, N = m.b, m.N
    before, mass, d0 = m.spread()
    n = 4096
    arena, slot, _, got, _ = _global(b, 2, n, True)
    assert got == n and len(set(arena.tolist())) > N // 2 and (arena >= 1024).any()
    isz = b.TRANSITION_DTYPE.itemsize
    ar_d, sl_d = DeviceBuffer(4 * n).upload(arena), DeviceBuffer(4 * n).upload(slot)
    rows_l = DeviceBuffer(n * isz)
    b.replay_gather_list_into(ar_d, sl_d, n, rows_l, None, None)
    tab, per, batch = _table(arena, slot, N)
    tab_d, per_d = DeviceBuffer(tab.nbytes).upload(tab), DeviceBuffer(per.nbytes).upload(per)
    rows_w, got_w = rc.gather_rows(b, tab_d, per_d, batch, 0, n)
    b.sync()
    listed = rows_l.download(b.TRANSITION_DTYPE, (n,))
    assert got_w == n and listed.tobytes() == rows_w.download(b.TRANSITION_DTYPE, (n,)).tobytes()
    assert listed.tobytes() == m.rows[arena, slot].tobytes()
    key = arena.astype(np.int64) * 2 ** 20 + slot
    dups = np.flatnonzero(np.diff(key) == 0)
    assert len(dups) >= 2, "too few duplicate draws to test the last-write rule"
    td = np.random.RandomState(N).normal(0, 3, (n, 2)).astype(np.float32)
    td[dups[0] + 1, 0] = np.nan                          # the later entry of a duplicated row is skipped: the earlier stays
    td[5, 1], td[9, 0] = np.inf, -np.inf
    j_top = n // 2 if n // 2 != dups[0] + 1 else n // 2 + 1
    td[j_top, 0] = 5000.0                                # one mass above every other: the maximum all arenas must take
    td_d = DeviceBuffer(td.nbytes).upload(td)
    mmax0 = d0["mmax"]
    assert len(set(mmax0.tolist())) > 1 and mmax0[0] == 1.0, "the running maxima are already level"
    b.replay_update_priorities_list(ar_d, sl_d, n, rows_l.ptr, td_d.ptr)
    b.sync()
    want, want_max = gso.write_back(mass, mmax0, arena, slot, [True] * n, td, 1.0, 1e-3)
    _, after, d = _snapshot(b)
    print("replay-scale mmax %s: read from an export of %d segments" % (m.case, -(-2 * N * b.replay_frames // SEG)))
    changed = 0
    for a in range(N):
        got_m, was = after[a, :m.cnt[a]], before[a, :m.cnt[a]]
        assert (np.abs(got_m - want[a]) <= 2 * np.spacing(want[a].astype(np.float32))).all(), a
        same = want[a] == was
        assert np.array_equal(got_m[same], was[same])                      # not written: bit-identical
        changed += int((~same).sum())
    assert changed > 1024
    for a in m.spot:
        assert np.array_equal(after[a, :m.cnt[a]], b.replay_priorities(a)), a
    top = np.float32(per_oracle.new_mass(5000.0, td[j_top, 1], 1.0, 1e-3))
    assert want_max[0] == max(want_max) and abs(np.float32(want_max[0]) - top) <= 2 * np.spacing(top)
    assert abs(d["mmax"][arena[j_top]] - top) <= 2 * np.spacing(top)
    assert (d["mmax"] == d["mmax"][arena[j_top]]).all(), np.flatnonzero(d["mmax"] != d["mmax"][arena[j_top]])[:8]
