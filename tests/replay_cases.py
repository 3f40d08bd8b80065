"""What the replay-memory tests share on the device: the collecting rollout on any map size, capture masks that leave
arenas with 0, 1, 4 and 11 rows, the wide memory whose arenas hold more rows than the samplers have chunks, the rows of a
window without their maps, hand-set masses, and how many of an arena's oldest rows lost their frame.  A helper module
(not collected)."""
import ctypes as C

import numpy as np


def varied_masks(NG, M):
    """arena 0 never captures (0 rows), arena 1 captures at ticks 0-1 (1 row), arena 2 with one ship (11 rows at 12
    ticks), arena 3 one ship at ticks 0-4 (4 rows), the others every ship."""
    def masks(t):
        mk = np.ones((NG, M), np.uint8)
        mk[0] = 0
        mk[1] = 0
        mk[1, 0] = t < 2
        mk[2] = 0
        mk[2, 0] = 1
        mk[3] = 0
        mk[3, 0] = t < 5
        return mk
    return masks


def rollout(N, M=4, capacity=40, frames=0, ticks=12, seed=0x0F160011, arena_base=0, prioritize=True, alpha=0.6,
            masks=None, packed=False, restart_every=0, width=400, height=400, ship_radius=None, laser_radius=None,
            pool_pairs=0, after_spawn=None):
    """A seeded collecting rollout with capture on a width x height map; masks(t) -> uint8 [N_global][M] of the
    capturing ships at tick t; restart_every: a new episode every so many lock-steps (0 = one episode); packed /
    pool_pairs: the frame store; after_spawn(b) runs after the spawn and after every restart (to place ships)."""
    from ofighters_amd import ArenaBatch, DeviceBuffer
    cfg = dict(width=width, height=height, arena_base=arena_base)
    if ship_radius is not None:
        cfg["ship_radius"] = ship_radius
    if laser_radius is not None:
        cfg["laser_radius"] = laser_radius
    b = ArenaBatch(N, M, **cfg)
    b.replay_create(capacity, frames, packed=packed, pool_pairs=pool_pairs)
    if prioritize:
        b.replay_prioritize(alpha, 1e-3)
    b.spawn_random(seed)
    if after_spawn:
        after_spawn(b)
    ia_d, ip_d = DeviceBuffer(4 * N * M), DeviceBuffer(8 * N * M)
    mask_d = DeviceBuffer(N * M)
    for t in range(ticks):
        mk = np.ones((N, M), np.uint8) if masks is None else masks(t)[arena_base:arena_base + N]
        b.sync()
        if restart_every and t and t % restart_every == 0:
            b.restart_random(seed)
            if after_spawn:
                after_spawn(b)
        mask_d.upload(np.ascontiguousarray(mk))
        b.bot_actions(["random"] * M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, ship_mask_ptr=mask_d.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, mask_d.ptr, ia_d.ptr, ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()
    return b


WIDE_N, WIDE_M, WIDE_CAPACITY, WIDE_TICKS, WIDE_RESTART, WIDE_FRAMES = 8, 8, 200, 70, 10, 24
_WIDE_SHIPS = (0, 8, 6, 4, 3, 2, 1, 8)


def wide_masks(NG=WIDE_N, M=WIDE_M):
    """The memory of WIDE_CAPACITY rows the samplers are held to beyond one row per chunk: arena a captures with its
    first _WIDE_SHIPS[a] ships (arena 0 never), the last arena only before lock-step 25, so that its frame ring stands
    still while it holds more than 128 eligible rows.  With a new episode every WIDE_RESTART lock-steps the ships come
    back, the busy arenas' row rings wrap within WIDE_TICKS lock-steps, and a ring of WIDE_FRAMES frames expires more
    than 64 of their oldest rows."""
    assert (NG, M) == (WIDE_N, WIDE_M)
    def masks(t):
        mk = np.zeros((NG, M), np.uint8)
        for a, k in enumerate(_WIDE_SHIPS):
            mk[a, :k] = 1
        if t >= 25:
            mk[NG - 1] = 0
        return mk
    return masks


def wide_preconditions(cnt, appended, skip, frames, batch=None):
    """What a wide memory must hold for its test to reach the code one row per chunk never reaches.  cnt / appended
    [N] of replay_count, skip [N] expired oldest rows.  Prints the figures before it asserts."""
    C = WIDE_CAPACITY
    cnt, skip = np.asarray(cnt, np.int64), np.asarray(skip, np.int64)
    valid = cnt - skip
    first = (np.asarray(appended, np.int64) % C - cnt) % C   # head = appended % C
    cs = -(-valid // 64)
    print("wide memory: count %s skip %s valid %s first %s" % (cnt.tolist(), skip.tolist(), valid.tolist(), first.tolist()))
    assert (cnt == C).any() and (appended > C).any(), "no row ring wrapped"
    assert (valid >= 129).any(), "no arena with chunks of three rows"
    assert ((valid >= 65) & (valid <= 128)).any(), "no arena with chunks of two rows"
    assert ((valid > 0) & (valid % np.maximum(cs, 1) != 0)).any(), "no ragged last chunk"
    assert ((valid > 0) & (first + skip + valid > C)).any(), "no arena whose eligible rows wrap the ring"
    if frames:
        assert (skip >= 65).any(), "no expiry walk of more than 64 rows"
    else:
        assert (skip == 0).all()
    if batch is not None and batch > 64:
        assert (valid >= batch).any(), "no arena draws more than 64 rows"


def gather_rows(b, slot, n_s, batch, first, max_rows):
    """gather_valid without the maps -> (rows DeviceBuffer, n_rows)."""
    from ofighters_amd import DeviceBuffer, _native as nat
    rows = DeviceBuffer(max(1, max_rows) * b.TRANSITION_DTYPE.itemsize)
    n = C.c_int32()
    nat.check(nat.lib().ofx_replay_gather_valid(b.handle, slot.ptr, n_s.ptr, int(batch), int(first), int(max_rows), rows.ptr,
                                                 None, None, C.byref(n)))
    return rows, n.value


def all_rows_window(b):
    """slot / n_sampled naming every row of every arena (oldest first), and those rows gathered."""
    from ofighters_amd import DeviceBuffer
    cnt, _ = b.replay_count()
    Cap = b.replay_capacity
    slot = np.full((b.N, Cap), -1, np.int32)
    for a in range(b.N):
        slot[a, :cnt[a]] = np.arange(cnt[a])
    slot_d, n_d = DeviceBuffer(slot.nbytes).upload(slot), DeviceBuffer(4 * b.N).upload(cnt.astype(np.int32))
    total = int(cnt.sum())
    rows, got = gather_rows(b, slot_d, n_d, Cap, 0, total)
    assert got == total
    return slot_d, n_d, Cap, rows, total, cnt


def set_masses(b, td_fn):
    """Hand-set masses: one write-back over every row with td = td_fn(rows) [n][2]."""
    from ofighters_amd import DeviceBuffer
    slot_d, n_d, Cap, rows, total, cnt = all_rows_window(b)
    b.sync()
    r = rows.download(b.TRANSITION_DTYPE, (total,))
    td = np.ascontiguousarray(td_fn(r), np.float32)
    td_d = DeviceBuffer(td.nbytes).upload(td)
    b.replay_update_priorities(slot_d, n_d, Cap, 0, total, rows.ptr, td_d.ptr)
    b.sync()
    return r, td


def spread_masses(b, seed, heavy=()):
    """Hand-set masses over six decades: 10^U(-3, 3) per row (seeded) as the first TD error, the second zero.  heavy:
    arenas whose rows all sit at the top of that range, 1000, so that a stratified draw of a few thousand rows over the
    whole memory cannot pass them by."""
    rs = np.random.RandomState(seed)
    spread = 10.0 ** rs.uniform(-3, 3, b.N * b.replay_capacity)
    cnt, _ = b.replay_count()
    top = np.isin(np.repeat(np.arange(b.N), cnt), list(heavy))

    def td(r):
        e = spread[:len(r)].copy()
        e[top] = 1000.0
        return np.stack([e, np.zeros(len(r))], 1)
    return set_masses(b, td)


def stale_rows(b, a):
    """How many of the arena's oldest rows have lost their `state` frame (not eligible)."""
    from ofighters_amd import OfxError
    rows = b.replay_rows(a)
    for k, r in enumerate(rows):
        try:
            b.replay_frame(a, int(r["tick_prev"]))
            return k
        except OfxError:
            pass
    return len(rows)
