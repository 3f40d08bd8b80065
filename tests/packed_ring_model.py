"""numpy restatement of the packed frame store's bookkeeping (include/ofx.h, "packed frame store": steps 1-3 of the
storing rule and the import's placement) for ONE arena.  It never sees a pair, only how many each frame has: that is
all the rule depends on.  tests/test_packed_store.py unit-tests it with hand-made counts; tests/test_gpu_packed_store.py
replays the per-frame nonzero-word counts of a dense twin through it and compares the device with what it predicts."""
import numpy as np


class PackedRing:
    def __init__(self, frames, pool_pairs):
        self.F, self.pool = int(frames), int(pool_pairs)
        self.frame_tick = np.full(self.F, -1, np.int64)
        self.cnt = np.zeros((self.F, 2), np.int64)
        self.off = np.zeros(self.F, np.int64)
        self.frame_head = 0
        self.pool_head = 0
        self.live = 0
        self.evicted = 0

    def store(self, tick, k_ship, k_laser):
        """One stored frame (the arena had a playing agent on lock-step `tick`)."""
        s, k = self.frame_head, int(k_ship) + int(k_laser)
        assert 0 <= k <= self.pool // 2, "a frame has at most 2 * words pairs and the pool at least 4 * words"
        if self.frame_tick[s] >= 0:                              # 1. the slot ring has wrapped onto its oldest frame
            self.live -= int(self.cnt[s].sum())
            self.frame_tick[s] = -1
            self.cnt[s] = 0
        j = s
        while self.live + k > self.pool:                         # 2. early eviction, oldest first
            j = (j + 1) % self.F
            assert j != s, "the pool cannot be full of nothing"
            if self.frame_tick[j] < 0:
                continue
            self.live -= int(self.cnt[j].sum())
            self.frame_tick[j] = -1
            self.cnt[j] = 0
            self.evicted += 1
        self.off[s] = self.pool_head                             # 3.
        self.cnt[s] = (k_ship, k_laser)
        self.pool_head = (self.pool_head + k) % self.pool
        self.live += k
        self.frame_tick[s] = tick
        self.frame_head = (s + 1) % self.F

    def live_ticks(self):
        return sorted(int(t) for t in self.frame_tick if t >= 0)

    def ranges(self):
        """{tick: set of the pool positions its pairs occupy}."""
        return {int(self.frame_tick[s]): {(int(self.off[s]) + i) % self.pool for i in range(int(self.cnt[s].sum()))}
                for s in range(self.F) if self.frame_tick[s] >= 0}

    def repacked(self):
        """The import's placement of this memory's live frames: chronological from pool position 0.  None when they do
        not fit (they always do for a memory this rule produced under the same pool)."""
        r = PackedRing(self.F, self.pool)
        r.frame_tick, r.cnt, r.frame_head, r.evicted = self.frame_tick.copy(), self.cnt.copy(), self.frame_head, 0
        pos = 0
        for i in range(self.F):
            s = (self.frame_head + i) % self.F
            if self.frame_tick[s] < 0:
                continue
            r.off[s] = pos % self.pool
            pos += int(self.cnt[s].sum())
        if pos > self.pool:
            return None
        r.live, r.pool_head = pos, pos % self.pool
        return r


def eligible(rows, frame_tick):
    """How many of an arena's rows (oldest first, the structured array of ArenaBatch.replay_rows) the samplers may draw:
    the oldest rows whose `state` frame has left the store are skipped."""
    skip = 0
    while skip < len(rows) and frame_tick[rows["frame_prev"][skip]] != rows["tick_prev"][skip]:
        skip += 1
    return len(rows) - skip
