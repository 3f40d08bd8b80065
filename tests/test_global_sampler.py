"""Global minibatch sampling (include/ofx.h, "global minibatch sampling"): the CPU restatement's properties and
DeviceTrainer's argument checks, and on the GPU the sampler against the restatement, the list gather against the window
gathers and the list write-back against the per-arena write-back."""
import ctypes as C

import numpy as np
import pytest
from scipy import stats

from tests import global_sample_oracle as gso
from tests import per_oracle
from tests import replay_cases as _wide

GLOBAL_SYMBOLS = ["ofx_replay_sample_global", "ofx_replay_gather_list", "ofx_replay_update_priorities_list"]
W = H = 400
WORDS = W * H // 32


# ------------------------------------------------------------------------------------------------------ CPU
def test_global_symbols_exported_declared_and_bound():
    from ofighters_amd import _native as nat
    from tests.abi_header import header_symbols
    L = C.CDLL(nat.LIB_PATH)
    declared = header_symbols()
    for s in GLOBAL_SYMBOLS:
        assert s in declared and s in nat.SIGNATURES and hasattr(L, s), s


def test_restatement_strata_are_disjoint_and_cover():
    for R in (1, 2, 7, 64, 257, 11840, 2 ** 31 - 1):
        for n in (1, 2, 7, 64, 256, R):
            if n > R or n > 20000:
                continue
            st = gso.strata(R, n)
            assert st[0][0] == 0 and st[-1][1] == R
            assert all(lo < hi for lo, hi in st)                                   # n <= R: no stratum is empty
            assert all(st[j][1] == st[j + 1][0] for j in range(n - 1))             # disjoint, no gap


def test_restatement_uniform_returns_every_row_once_and_ascending():
    v, skip = [0, 1, 11, 4, 40, 0, 3], [0, 0, 0, 2, 5, 7, 0]
    R = sum(v)
    want = [(a, skip[a] + i) for a in range(len(v)) for i in range(v[a])]
    for n_rows in (R, R + 5):
        arena, slot, n, gotR = gso.sample_uniform(v, skip, n_rows, 9, 2, 0)
        assert (n, gotR) == (R, R) and list(zip(arena, slot)) == want
    for n_rows in (1, 7, 20):
        for d in range(20):
            arena, slot, n, _ = gso.sample_uniform(v, skip, n_rows, 9, 2, d)
            pairs = list(zip(arena, slot))
            assert n == n_rows and pairs == sorted(set(pairs)) and set(pairs) <= set(want)
    assert gso.sample_uniform([0, 0], [0, 3], 4, 9, 0, 0) == ([], [], 0, 0)
    # the arena offset keys the stream: two shards draw different rows from equal memories
    assert gso.sample_uniform(v, skip, 7, 9, 0, 0)[:2] != gso.sample_uniform(v, skip, 7, 9, 100, 0)[:2]


def test_restatement_uniform_frequencies_are_uniform_over_rows():
    """A row is drawn with probability 1 / (size of its stratum): n / R exactly when n divides R, else within the
    rounding of the strata's integer bounds."""
    v, skip = [3, 0, 17, 1, 9], [1, 0, 0, 0, 2]
    rows = [(a, skip[a] + i) for a in range(len(v)) for i in range(v[a])]
    R = len(rows)
    for n_rows in (5, 4):                                # 30 rows: strata of 6 rows each / of 7, 8, 7 and 8 rows
        counts = dict.fromkeys(rows, 0)
        for d in range(3000):
            arena, slot, _, _ = gso.sample_uniform(v, skip, n_rows, 21, 0, d)
            for k in zip(arena, slot):
                counts[k] += 1
        expect = np.concatenate([np.full(hi - lo, 3000.0 / (hi - lo)) for lo, hi in gso.strata(R, n_rows)])
        assert n_rows != 5 or (expect == 500).all()
        assert abs(expect / 3000 - n_rows / R).max() <= (n_rows / R) ** 2 * 1.5      # within one row per stratum
        assert stats.chisquare(list(counts.values()), expect).pvalue > 1e-3


def test_restatement_prioritized_frequencies_follow_the_masses_across_arenas():
    rs = np.random.RandomState(3)
    sizes, skip = [5, 0, 12, 1, 9, 7], [2, 0, 0, 0, 3, 0]
    mass = [(10.0 ** rs.uniform(-1, 1, k)).astype(np.float32) for k in sizes]
    rows = [(a, i) for a in range(len(sizes)) for i in range(skip[a], sizes[a])]
    counts = dict.fromkeys(rows, 0)
    for d in range(2500):
        arena, slot, w, n, R = gso.sample_prioritized(mass, skip, 8, 0.4, 0x0F160005, 3, d)
        assert n == 8 and R == len(rows) and w.max() == 1.0 and (w > 0).all()
        pairs = list(zip(arena, slot))
        assert pairs == sorted(pairs)                                              # non-decreasing: duplicates adjacent
        for k in pairs:
            counts[k] += 1                                                         # (an expired row would be a KeyError)
    m = np.array([float(mass[a][i]) for a, i in rows])
    assert stats.chisquare(list(counts.values()), 20000 * m / m.sum()).pvalue > 1e-3


def test_restatement_weights_correct_to_uniform_over_rows():
    mass = [np.array([1, 4], np.float32), np.array([2, 1, 8, 0.5], np.float32)]
    for beta in (0.0, 0.4, 1.0):
        arena, slot, w, n, R = gso.sample_prioritized(mass, [0, 1], 16, beta, 1, 0, 0)
        total = 1 + 4 + 1 + 8 + 0.5
        raw = np.array([(R * float(mass[a][s]) / total) ** -beta for a, s in zip(arena, slot)], np.float32)
        np.testing.assert_array_equal(w, raw / raw.max())
    arena, slot, w, n, R = gso.sample_prioritized([np.ones(3, np.float32), np.ones(6, np.float32)], [0, 0], 9, 0.7, 1, 0, 0)
    assert sorted(zip(arena, slot)) == [(0, i) for i in range(3)] + [(1, i) for i in range(6)] and (w == 1.0).all()


def test_restatement_group_scan_is_monotone():
    rs = np.random.RandomState(8)
    T = 10.0 ** rs.uniform(-3, 3, 1000)
    T[rs.randint(0, 1000, 100)] = 0.0                                              # empty arenas
    T[255:258] = 0.0                                                               # across the group boundary
    G = gso.group_scan(T)
    assert len(G) == 1000 and all(G[i] <= G[i + 1] for i in range(999))
    assert G[255] == G[256] == G[257]
    assert abs(G[-1] - T.sum()) <= 1e-9 * T.sum()
    s = 0.0
    for t in T[:256]:
        s += t
    assert G[255] == s and G[511] == s + sum_seq(T[256:512])                       # X_1 = s_last(0); G = X_k + s_a


def sum_seq(x):
    s = 0.0
    for t in x:
        s += float(t)
    return s


def test_restatement_write_back_levels_and_the_later_entry_wins():
    mass = [np.ones(3), np.ones(2), np.ones(0)]
    arena, slot = [0, 0, 0, 1, 1], [1, 1, 2, 0, 0]
    td = np.array([[5, 0], [2, 0], [np.nan, 1], [3, 0], [np.inf, 0]], np.float32)
    got, mmax = gso.write_back(mass, [1.0, 1.0, 1.0], arena, slot, [True, True, True, True, True], td, 1.0, 0.0)
    assert list(got[0]) == [1.0, 2.0, 1.0] and list(got[1]) == [3.0, 1.0]      # later finite entry; non-finite skipped
    assert mmax == [5.0, 5.0, 5.0]                                                # the losing entry raised mmax too
    got, mmax = gso.write_back(mass, [1.0, 1.0, 1.0], arena, slot, [False] * 5, td, 1.0, 0.0)
    assert all((g == 1.0).all() for g in got) and mmax == [1.0] * 3


def test_trainer_argument_checks(monkeypatch):
    from ofighters_amd.trainer import DeviceTrainer, fingerprint_diff
    from tests.checkpoint_standin import TRAINER_KEYS, host_trainer as _trainer
    with pytest.raises(ValueError) as err:
        DeviceTrainer(None, np.zeros(4, np.float32), global_sampling=True, reference_quirks=True)
    assert "global sampling" in str(err.value)
    for bad in (1, 0, None, "yes", 1.0):
        with pytest.raises(ValueError) as err:
            DeviceTrainer(None, np.zeros(4, np.float32), global_sampling=bad)
        assert "global_sampling" in str(err.value)
    off, on = _trainer(monkeypatch), _trainer(monkeypatch, global_sampling=True)
    assert off.global_sampling is False and on.global_sampling is True
    assert "global_sampling" not in off.fingerprint() and tuple(sorted(off.fingerprint())) == tuple(sorted(TRAINER_KEYS))
    assert on.fingerprint()["global_sampling"] is True
    assert fingerprint_diff(off.fingerprint(), on.fingerprint()) == ["global_sampling"]
    assert fingerprint_diff(on.fingerprint(), off.fingerprint()) == ["global_sampling"]
    for a, b in ((off, on), (on, off)):                  # a state taken under one sampler is refused under the other
        with pytest.raises(ValueError) as err:
            b.load_state_dict(a.state_dict())
        assert "global_sampling" in str(err.value)
    on.load_state_dict(on.state_dict())


# ------------------------------------------------------------------------------------------------------ GPU
def _rollout(N, M=4, capacity=40, frames=0, ticks=12, seed=0x0F160011, arena_base=0, prioritize=True, alpha=0.6,
             masks=None, packed=False, restart_every=0):
    """A seeded collecting rollout with capture; masks(t) -> uint8 [N_global][M] of the capturing ships at tick t
    (tests/test_prioritized_replay.py's helper, with the choice of the frame store)."""
    return _wide.rollout(N, M, capacity=capacity, frames=frames, ticks=ticks, seed=seed, arena_base=arena_base,
                         prioritize=prioritize, alpha=alpha, masks=masks, packed=packed, restart_every=restart_every)


def _capture_more(b, ticks, seed=3):
    from ofighters_amd import DeviceBuffer
    ia_d, ip_d = DeviceBuffer(4 * b.N * b.M), DeviceBuffer(8 * b.N * b.M)
    for t in ticks:
        b.bot_actions(["random"] * b.M, seed, tick=t)
        b.policy_explore(1.0, seed, tick=t, collecting=True, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.replay_capture(t, None, ia_d.ptr, ip_d.ptr)
        b.policy_actions(out_ptr=b._actions.ptr, iaction_ptr=ia_d.ptr, ipointer_ptr=ip_d.ptr)
        b.step(actions_ptr=b._actions.ptr)
    b.sync()


def _eligibility(b):
    """(skip [N], v [N]) as ofx_replay_sample sees them: a per-arena draw of `capacity` rows returns every eligible row."""
    _, n = b.replay_sample(1, 0, b.replay_capacity)
    b.sync()
    v = n.download(np.int32, (b.N,))
    cnt, _ = b.replay_count()
    return (cnt - v).astype(int).tolist(), v.astype(int).tolist()


def _dev_sample(b, seed, draw, n_rows, per=False, beta=0.0):
    arena, slot, w, n, R = b.replay_sample_global(seed, draw, n_rows, per, beta)
    b.sync()
    return (arena.download(np.int32, (n_rows,)), slot.download(np.int32, (n_rows,)),
            w.download(np.float32, (n_rows,)) if w is not None else None, n, R, (arena, slot, w))


def _spread_masses(b, seed):
    _wide.spread_masses(b, seed)


_BETA = 0.4
_SEED = 0x0F160051


def _check_sampler(b, skip, v, n_rows_list, draws, arena_base=0):
    mass = [b.replay_priorities(a) for a in range(b.N)]
    R = sum(v)
    for n_rows in n_rows_list:
        for d in draws:
            arena, slot, w, n, gotR, _ = _dev_sample(b, _SEED, d, n_rows)
            ra, rs_, rn, rR = gso.sample_uniform(v, skip, n_rows, _SEED, arena_base, d)
            assert (n, gotR) == (rn, rR) == (min(n_rows, R), R)
            assert np.array_equal(arena[:n], ra) and np.array_equal(slot[:n], rs_), (n_rows, d)
            assert (arena[n:] == -1).all() and (slot[n:] == -1).all()
            key = arena[:n].astype(np.int64) * 2 ** 20 + slot[:n]
            assert (np.diff(key) > 0).all()                                        # strictly ascending: no row twice
            arena, slot, w, n, gotR, _ = _dev_sample(b, _SEED, d, n_rows, True, _BETA)
            ra, rs_, rw, rn, rR = gso.sample_prioritized(mass, skip, n_rows, _BETA, _SEED, arena_base, d)
            assert (n, gotR) == (rn, rR) == (min(n_rows, R), R)
            assert np.array_equal(arena[:n], ra) and np.array_equal(slot[:n], rs_), (n_rows, d)
            assert (arena[n:] == -1).all() and (slot[n:] == -1).all() and (w[n:] == 0).all()
            np.testing.assert_allclose(w[:n], rw, rtol=1e-6, atol=0, err_msg="n_rows %d draw %d" % (n_rows, d))
            key = arena[:n].astype(np.int64) * 2 ** 20 + slot[:n]
            assert (np.diff(key) >= 0).all()


# N == WIDE_N: the memory of tests/replay_cases.py's wide_masks - chunks of more than one row, ragged last chunks, a
# second round of the expiry walk and eligible rows across the ring's end
@pytest.mark.gpu
@pytest.mark.parametrize("N,frames,packed", [
    pytest.param(N, frames, packed, id="%d-%d-%s" % (N, frames, packed))
    for packed in (False, True) for frames in (0, 4) for N in (5, 300)] + [
    pytest.param(_wide.WIDE_N, frames, packed, id="wide-%d-%s" % (frames, packed))
    for frames, packed in ((0, False), (_wide.WIDE_FRAMES, False), (_wide.WIDE_FRAMES, True))])
def test_sampler_equals_restatement(N, frames, packed):
    from tests.replay_cases import stale_rows as _skip, varied_masks as _varied_masks
    wide = N == _wide.WIDE_N
    if wide:
        M = _wide.WIDE_M
        b = _rollout(N, M, capacity=_wide.WIDE_CAPACITY, frames=frames, ticks=_wide.WIDE_TICKS, masks=_wide.wide_masks(),
                     alpha=1.0, packed=packed, restart_every=_wide.WIDE_RESTART)
    else:
        M = 4
        b = _rollout(N, M, capacity=40, frames=frames, masks=_varied_masks(N, M), alpha=1.0, packed=packed)
        cnt, _ = b.replay_count()
        assert cnt[0] == 0 and cnt[1] == 1 and 0 < cnt[3] <= 4 < cnt[2] <= 11 and cnt[4] == 40 and (cnt == 40).sum() > (N - 4) // 2   # rings wrapped
    _spread_masses(b, N + frames)
    allm = np.concatenate([b.replay_priorities(a) for a in range(min(N, 16))])
    assert allm.max() / allm.min() > 1e5                                           # six decades (alpha = 1)
    skip, v = _eligibility(b)
    if wide:
        _wide.wide_preconditions(*b.replay_count(), skip, frames)
    if N == 5 or wide:
        assert skip == [_skip(b, a) for a in range(N)]                             # the host inspections agree
    if frames:
        assert max(skip) > 0, "no row expired"
    else:
        assert max(skip) == 0
    R = sum(v)
    assert R > 0 and v[0] == 0
    _check_sampler(b, skip, v, [1, 7, 64, 256, R, R + 5], range(3))
    b.close()


@pytest.mark.gpu
def test_shards_draw_different_rows_from_equal_memories():
    N, M = 5, 4
    from tests.replay_cases import varied_masks as _varied_masks
    a = _rollout(N, M, masks=_varied_masks(N, M), alpha=1.0)
    _spread_masses(a, 1)
    blob = a.replay_export(0, N)
    from ofighters_amd import ArenaBatch
    b = ArenaBatch(N, M, arena_base=64)
    b.replay_create(40, 0)
    b.replay_prioritize(1.0, 1e-3)
    b.spawn_random(1)
    b.replay_import(0, N, blob)
    assert all(np.array_equal(a.replay_priorities(x), b.replay_priorities(x)) and
               a.replay_rows(x).tobytes() == b.replay_rows(x).tobytes() for x in range(N))
    skip, v = _eligibility(a)
    assert (skip, v) == _eligibility(b)
    for per in (False, True):
        xa = _dev_sample(a, _SEED, 0, 7, per, _BETA)
        xb = _dev_sample(b, _SEED, 0, 7, per, _BETA)
        assert xa[3:5] == xb[3:5] == (7, sum(v))
        assert not (np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1]))
    _check_sampler(b, skip, v, [7], [0], arena_base=64)
    a.close(), b.close()


@pytest.mark.gpu
def test_sampler_on_an_empty_memory_and_argument_checks():
    from ofighters_amd import ArenaBatch, DeviceBuffer, OfxError, _native as nat
    b = ArenaBatch(3, 4)
    b.replay_create(40, 0)
    b.spawn_random(1)
    arena, slot, w, n, R, _ = _dev_sample(b, 1, 0, 4)
    assert (n, R) == (0, 0) and (arena == -1).all() and (slot == -1).all() and w is None
    with pytest.raises(OfxError) as err:                                           # PER is off
        b.replay_sample_global(1, 0, 4, True, 0.4)
    assert err.value.code == nat.OFX_ERR_STATE
    b.replay_prioritize(0.6, 1e-3)
    arena, slot, w, n, R, _ = _dev_sample(b, 1, 0, 4, True, 0.4)
    assert (n, R) == (0, 0) and (arena == -1).all() and (w == 0).all()
    buf = DeviceBuffer(64)
    n_h, e_h = C.c_int32(), C.c_int64()
    L = nat.lib()
    for args in ((1, 0, 0, 0, 0.0, buf.ptr, buf.ptr, None), (1, 0, 4, 1, 0.4, buf.ptr, buf.ptr, None),
                 (1, 0, 4, 1, float("nan"), buf.ptr, buf.ptr, buf.ptr), (1, 0, 4, 0, 0.0, None, buf.ptr, None)):
        assert L.ofx_replay_sample_global(b.handle, *args, C.byref(n_h), C.byref(e_h)) == nat.OFX_ERR_INVALID
    rows = DeviceBuffer(4 * b.TRANSITION_DTYPE.itemsize)
    for n_, nstep, gamma, ret in ((0, 1, 0.9, None), (4, 0, 0.9, None), (4, 65, 0.9, buf.ptr), (4, 3, 1.5, buf.ptr),
                                  (4, 3, float("nan"), buf.ptr), (4, 3, 0.9, None)):
        assert L.ofx_replay_gather_list(b.handle, buf.ptr, buf.ptr, n_, nstep, gamma, rows.ptr, None, None, ret,
                                        ret) == nat.OFX_ERR_INVALID
    b.close()


# ---- the list gather --------------------------------------------------------------------------------------------------
def _table(arena, slot, N):
    """The slot[N][batch] / n_sampled[N] table whose packed (arena, j) order is the sorted list."""
    per = np.bincount(arena, minlength=N)
    batch = int(per.max())
    tab = np.full((N, batch), -1, np.int32)
    fill = np.zeros(N, int)
    for a, s in zip(arena, slot):
        tab[a, fill[a]] = s
        fill[a] += 1
    return tab, per.astype(np.int32), batch


def _gather_both(b, arena_h, slot_h, nstep, gamma=0.9):
    """The list gather and the window gather of the same rows -> two tuples (rows, bits_prev, bits_next, ret, disc)."""
    from ofighters_amd import DeviceBuffer
    n = len(arena_h)
    tab, per, batch = _table(arena_h, slot_h, b.N)
    isz = b.TRANSITION_DTYPE.itemsize
    mk = lambda: (DeviceBuffer(n * isz), DeviceBuffer(8 * n * WORDS), DeviceBuffer(8 * n * WORDS), DeviceBuffer(4 * n),
                  DeviceBuffer(4 * n))
    A, B = mk(), mk()
    ar_d = DeviceBuffer(4 * n).upload(np.ascontiguousarray(arena_h, np.int32))
    sl_d = DeviceBuffer(4 * n).upload(np.ascontiguousarray(slot_h, np.int32))
    tab_d, per_d = DeviceBuffer(tab.nbytes).upload(tab), DeviceBuffer(per.nbytes).upload(per)
    if nstep is None:
        b.replay_gather_list_into(ar_d, sl_d, n, A[0], A[1], A[2])
        got = b.replay_gather_valid_into(tab_d, per_d, batch, 0, n, B[0], B[1], B[2])
    else:
        b.replay_gather_list_into(ar_d, sl_d, n, A[0], A[1], A[2], nstep, gamma, A[3], A[4])
        got = b.replay_gather_nstep_into(tab_d, per_d, batch, 0, n, nstep, gamma, B[0], B[1], B[2], B[3], B[4])
    assert got == n
    b.sync()
    dl = lambda X: (X[0].download(b.TRANSITION_DTYPE, (n,)), X[1].download(np.uint32, (n, 2, WORDS)),
                    X[2].download(np.uint32, (n, 2, WORDS)),
                    None if nstep is None else X[3].download(np.float32, (n,)),
                    None if nstep is None else X[4].download(np.float32, (n,)))
    return dl(A), dl(B)


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_list_gather_equals_the_window_gathers(packed):
    from tests.replay_cases import varied_masks as _varied_masks
    N, M = 5, 4
    b = _rollout(N, M, capacity=40, frames=0, masks=_varied_masks(N, M), alpha=1.0, packed=packed)
    _spread_masses(b, 2)
    lists = []
    arena, slot, _, n, _, _ = _dev_sample(b, _SEED, 0, 24)
    lists.append((arena[:n], slot[:n]))
    arena, slot, _, n, _, _ = _dev_sample(b, _SEED, 1, 48, True, _BETA)
    assert (np.diff(arena[:n].astype(np.int64) * 2 ** 20 + slot[:n]) == 0).any(), "no duplicate draw in the list"
    lists.append((arena[:n], slot[:n]))
    chained = 0
    for arena_h, slot_h in lists:
        for nstep in (None, 1, 3):
            A, B = _gather_both(b, arena_h, slot_h, nstep)
            assert A[0].tobytes() == B[0].tobytes()
            assert np.array_equal(A[1], B[1]) and np.array_equal(A[2], B[2])
            assert A[1].any() and A[2].any()
            if nstep is not None:
                assert np.array_equal(A[3], B[3]) and np.array_equal(A[4], B[4])
            if nstep == 3:
                chained += int((A[0]["tick_next"] - A[0]["tick_prev"] > 1).sum())
    assert chained > 0, "no n-step chain went past one row"
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True])
def test_list_gather_pads_entries_that_name_no_row(packed):
    from ofighters_amd import DeviceBuffer
    from tests.replay_cases import varied_masks as _varied_masks
    N, M = 5, 4
    b = _rollout(N, M, capacity=40, frames=0, masks=_varied_masks(N, M), packed=packed)
    cnt, _ = b.replay_count()
    arena = np.array([-1, 0, 1, 1, 2, 3, 4, 4, N, 2 ** 31 - 1, -2 ** 31, 4], np.int32)
    slot = np.array([0, 0, 0, 1, -1, int(cnt[3]), 39, 40, 0, 0, 0, 2 ** 31 - 1], np.int32)
    good = np.array([0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 0], bool)                # (1, 0) and (4, 39) name rows
    n = len(arena)
    isz = b.TRANSITION_DTYPE.itemsize
    for nstep in (1, 3):
        rows, bp, bn = DeviceBuffer(n * isz), DeviceBuffer(8 * n * WORDS), DeviceBuffer(8 * n * WORDS)
        ret, disc = DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        for buf in (rows, bp, bn, ret, disc):
            buf.upload(np.full(buf.nbytes, 0xAB, np.uint8))
        ar_d, sl_d = DeviceBuffer(4 * n).upload(arena), DeviceBuffer(4 * n).upload(slot)   # held until the sync
        b.replay_gather_list_into(ar_d, sl_d, n, rows, bp, bn, nstep, 0.9, ret, disc)
        b.sync()
        r = rows.download(b.TRANSITION_DTYPE, (n,))
        p, q = bp.download(np.uint32, (n, 2, WORDS)), bn.download(np.uint32, (n, 2, WORDS))
        pad = np.zeros(1, b.TRANSITION_DTYPE)
        pad["ship"] = -1
        for d in range(n):
            if good[d]:
                want = b.replay_rows(int(arena[d]))[int(slot[d])]
                assert r[d]["tick_prev"] == want["tick_prev"] and r[d]["ship"] == want["ship"] and p[d].any()
            else:
                assert r[d].tobytes() == pad[0].tobytes() and not p[d].any() and not q[d].any(), d
        assert (ret.download(np.float32, (n,))[~good] == 0).all() and (disc.download(np.float32, (n,))[~good] == 0).all()
    b.close()


# ---- the list write-back ---------------------------------------------------------------------------------------------
def _both_write_backs(a, b, arena_h, slot_h, td, between=None):
    """The same entries and td through the list write-back on memory a and the per-arena write-back on the equal memory
    b; `between` runs on both after the rows were gathered."""
    from ofighters_amd import DeviceBuffer
    n = len(arena_h)
    isz = a.TRANSITION_DTYPE.itemsize
    ar_d = DeviceBuffer(4 * n).upload(np.ascontiguousarray(arena_h, np.int32))
    sl_d = DeviceBuffer(4 * n).upload(np.ascontiguousarray(slot_h, np.int32))
    rows_a, rows_b = DeviceBuffer(n * isz), DeviceBuffer(n * isz)
    a.replay_gather_list_into(ar_d, sl_d, n, rows_a, None, None)
    tab, per, batch = _table(arena_h, slot_h, b.N)
    tab_d, per_d = DeviceBuffer(tab.nbytes).upload(tab), DeviceBuffer(per.nbytes).upload(per)
    from tests.replay_cases import gather_rows as _gather_rows
    rows_b, got = _gather_rows(b, tab_d, per_d, batch, 0, n)
    assert got == n
    a.sync(), b.sync()
    assert rows_a.download(a.TRANSITION_DTYPE, (n,)).tobytes() == rows_b.download(b.TRANSITION_DTYPE, (n,)).tobytes()
    if between:
        between(a), between(b)
    td = np.ascontiguousarray(td, np.float32)
    td_a, td_b = DeviceBuffer(td.nbytes).upload(td), DeviceBuffer(td.nbytes).upload(td)   # held until the sync below
    a.replay_update_priorities_list(ar_d, sl_d, n, rows_a.ptr, td_a.ptr)
    b.replay_update_priorities(tab_d, per_d, batch, 0, n, rows_b.ptr, td_b.ptr)
    a.sync(), b.sync()
    return [a.replay_priorities(x) for x in range(a.N)], [b.replay_priorities(x) for x in range(b.N)]


@pytest.mark.gpu
def test_list_write_back_equals_the_per_arena_write_back():
    from tests.replay_cases import varied_masks as _varied_masks
    N, M = 16, 4
    mems = []
    for _ in range(2):
        b = _rollout(N, M, capacity=40, masks=_varied_masks(N, M))
        _spread_masses(b, 4)
        mems.append(b)
    a, b = mems
    before = [a.replay_priorities(x) for x in range(N)]
    assert all(np.array_equal(before[x], b.replay_priorities(x)) for x in range(N))
    arena, slot, _, n, _, _ = _dev_sample(a, _SEED, 0, 96, True, _BETA)
    assert n == 96
    key = arena.astype(np.int64) * 2 ** 20 + slot
    dups = np.flatnonzero(np.diff(key) == 0)
    assert len(dups) >= 2, "too few duplicate draws to test the last-write rule"
    rs = np.random.RandomState(4)
    td = rs.normal(0, 3, (n, 2)).astype(np.float32)
    td[dups[0] + 1, 0] = np.nan                          # the later entry of a duplicated row is skipped: the earlier stays
    lone = [j for j in range(n) if (key == key[j]).sum() == 1][:2]
    td[lone[0], 1], td[lone[1], 0] = np.inf, -np.inf
    ma, mb = _both_write_backs(a, b, arena, slot, td)
    for x in range(N):
        assert np.array_equal(ma[x], mb[x]), x
    j = dups[1]                                          # a duplicated row keeps the later entry's priority
    want = np.float32(per_oracle.new_mass(td[j + 1, 0], td[j + 1, 1], 0.6, 1e-3))
    assert abs(ma[arena[j]][slot[j]] - want) <= 2 * np.spacing(want)
    assert ma[arena[lone[0]]][slot[lone[0]]] == before[arena[lone[0]]][slot[lone[0]]]          # non-finite: untouched
    j = dups[0]
    want = np.float32(per_oracle.new_mass(td[j, 0], td[j, 1], 0.6, 1e-3))
    assert abs(ma[arena[j]][slot[j]] - want) <= 2 * np.spacing(want)
    assert sum(int((ma[x] != before[x]).sum()) for x in range(N)) > 40
    a.close(), b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("full", [False, True])
def test_list_write_back_skips_rows_overwritten_since_sampling(full):
    N, M = 8, 4
    Cap = 24 if full else 200
    a, b = (_rollout(N, M, capacity=Cap, ticks=8) for _ in range(2))
    cnt0, app0 = a.replay_count()
    arena, slot, _, n, _, _ = _dev_sample(a, 3, 0, 64, True, _BETA)
    assert n == 64
    ma, mb = _both_write_backs(a, b, arena, slot, np.full((n, 2), 50.0, np.float32),
                               between=lambda x: _capture_more(x, (8, 9)))
    cnt1, app1 = a.replay_count()
    shifted = (cnt0 == Cap) & (app1 > app0)             # full memories that took new rows: every slot has moved
    assert shifted.any() == full
    big = np.float32(per_oracle.new_mass(50.0, 50.0, 0.6, 1e-3))
    landed = 0
    for x in range(N):
        assert np.array_equal(ma[x], mb[x]), x
        hit = np.abs(ma[x] - big) <= 2 * np.spacing(big)
        assert ((ma[x] == 1.0) | hit).all()
        if shifted[x]:
            assert not hit.any()                             # no priority landed on another row
        landed += int(hit.sum())
    if not full:
        assert landed == len(set(zip(arena.tolist(), slot.tolist())))
    a.close(), b.close()


@pytest.mark.gpu
def test_rows_captured_after_a_list_write_back_carry_the_global_maximum():
    from ofighters_amd import DeviceBuffer
    N, M = 8, 4
    b = _rollout(N, M, capacity=200, ticks=8)
    cnt, app = b.replay_count()
    assert cnt[2] >= 3
    arena, slot = np.array([2, 2, 2], np.int32), np.array([0, 1, 2], np.int32)      # entries in one arena only
    ar_d, sl_d = DeviceBuffer(12).upload(arena), DeviceBuffer(12).upload(slot)
    rows = DeviceBuffer(3 * b.TRANSITION_DTYPE.itemsize)
    b.replay_gather_list_into(ar_d, sl_d, 3, rows, None, None)
    td = np.array([[7, 0], [30, -2], [0.5, 0]], np.float32)
    td_d = DeviceBuffer(td.nbytes).upload(td)
    b.replay_update_priorities_list(ar_d, sl_d, 3, rows.ptr, td_d.ptr)
    b.sync()
    mass = [np.ones(int(c)) for c in cnt]
    want, mmax = gso.write_back(mass, [1.0] * N, arena, slot, [True] * 3, td, 0.6, 1e-3)
    top = np.float32(mmax[0])
    assert top > 1.0 and len(set(mmax)) == 1
    for x in range(N):
        got = b.replay_priorities(x).astype(np.float64)
        assert (np.abs(got - want[x]) <= 2 * np.spacing(want[x].astype(np.float32))).all()
    _capture_more(b, (8,))
    cnt2, app2 = b.replay_count()
    grew = app2 > app
    assert grew.sum() > N // 2 and grew[[x for x in range(N) if x != 2]].any()
    biggest = b.replay_priorities(2)[:3].max()
    assert abs(biggest - top) <= 2 * np.spacing(top)
    for x in range(N):
        new = b.replay_priorities(x)[cnt[x]:]
        assert len(new) == app2[x] - app[x] and (new == biggest).all(), x              # every arena: the global maximum
    b.close()
