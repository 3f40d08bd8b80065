// ofx_packed.h - host-side arithmetic of the packed frame store (include/ofx.h, "packed frame store"): plain C++, no HIP,
// so that a stand-alone program can run it under the sanitizers (tools/packed_place_check.cpp).
#pragma once
#include <stdint.h>
#include <string.h>

// pool_pairs of ofx_replay_create_packed: 0 = the default, otherwise checked against [4 * words, 2^31).
// Returns the pool size, or 0 when the request is refused (*low / *high receive the bounds it must lie in).
static inline int64_t ofx_packed_pool_pairs(int64_t requested, int32_t frames, int32_t words, int64_t *low, int64_t *high) {
  *low = 4 * (int64_t)words;
  *high = (int64_t)1 << 31;
  int64_t p = requested;
  if (p == 0) {  // 512 pairs per slot, and never below the bound that lets two worst-case frames lie side by side
    p = 512 * (int64_t)frames;
    if (p < *low) p = *low;
  }
  return (p >= *low && p < *high) ? p : 0;
}

// HBM bytes of the packed store of n arenas: pool + frame_off + frame_cnt + pool_head + live + evicted
static inline int64_t ofx_packed_store_bytes(int64_t n, int64_t frames, int64_t pool_pairs) {
  return n * (pool_pairs * 8 + frames * 4 + frames * 2 * 4 + 4 + 4 + 8);
}

// The import's placement.  For each of the chunk's n arenas the live frames (frame_tick >= 0) are laid out in
// chronological order - the slots walked cyclically from frame_head, the oldest first - from pool position 0:
// frame_off[a][slot] = the slot's first pair, live[a] = the arena's pairs, pool_head[a] = live[a] mod pool_pairs.
// frame_tick [n][F] int32, frame_head [n] int32 and counts [n][F][2] uint32 are read bytewise (a blob sits at any
// alignment) and are what ofx_replay_blob_check has accepted: frame_head in [0, F), empty slots with count 0.
// Returns -1, or the first arena whose live pairs exceed pool_pairs (*need = its pairs): nothing may then be imported.
static inline int ofx_packed_place(int32_t n, int32_t F, int64_t pool_pairs, const uint8_t *frame_tick,
                                   const uint8_t *frame_head, const uint8_t *counts, uint32_t *frame_off,
                                   uint32_t *pool_head, uint32_t *live, int64_t *need) {
  for (int32_t a = 0; a < n; a++) {
    int32_t fh;
    memcpy(&fh, frame_head + 4 * (size_t)a, 4);
    int64_t pos = 0;
    for (int32_t i = 0; i < F; i++) {
      const size_t s = (size_t)a * F + (size_t)((fh + i) % F);
      int32_t tick;
      uint32_t c[2];
      memcpy(&tick, frame_tick + 4 * s, 4);
      memcpy(c, counts + 8 * s, 8);
      frame_off[s] = 0;
      if (tick < 0) continue;
      frame_off[s] = (uint32_t)(pos % pool_pairs);
      pos += (int64_t)c[0] + c[1];
    }
    if (pos > pool_pairs) {
      *need = pos;
      return a;
    }
    live[a] = (uint32_t)pos;
    pool_head[a] = (uint32_t)(pos % pool_pairs);
  }
  return -1;
}
