// Host logic of the packed frame store (ofighters_amd/csrc/ofx_packed.h) under AddressSanitizer and UBSan: the import's
// chronological placement, its pool-capacity refusal, and the pool_pairs bounds.  CPU only, no HIP, its own main:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o packed_place_check tools/packed_place_check.cpp
//   ./packed_place_check            (prints "packed_place_check ok", exit status 0)
// The blob arrays are handed over at odd addresses on purpose: a blob read from a file sits at any alignment.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../ofighters_amd/csrc/ofx_packed.h"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

struct Chunk {
  int n, F;
  std::vector<int32_t> tick, head;
  std::vector<uint32_t> cnt;
};

// exactly-sized heap copies at offset 1 of their allocation: an out-of-range read or a misaligned typed access is caught
static int place(const Chunk &c, int64_t pool, std::vector<uint32_t> &off, std::vector<uint32_t> &ph, std::vector<uint32_t> &live,
                 int64_t *need) {
  const size_t nt = 4 * c.tick.size(), nh = 4 * c.head.size(), nc = 4 * c.cnt.size();
  uint8_t *t = (uint8_t *)malloc(nt + 1), *h = (uint8_t *)malloc(nh + 1), *k = (uint8_t *)malloc(nc + 1);
  memcpy(t + 1, c.tick.data(), nt);
  memcpy(h + 1, c.head.data(), nh);
  memcpy(k + 1, c.cnt.data(), nc);
  off.assign((size_t)c.n * c.F, 0xDEADu);
  ph.assign(c.n, 0xDEADu);
  live.assign(c.n, 0xDEADu);
  const int rc = ofx_packed_place(c.n, c.F, pool, t + 1, h + 1, k + 1, off.data(), ph.data(), live.data(), need);
  free(t);
  free(h);
  free(k);
  return rc;
}

int main() {
  int64_t low, high;
  CHECK(ofx_packed_pool_pairs(0, 502, 5000, &low, &high) == 512 * 502 && low == 20000 && high == ((int64_t)1 << 31));
  CHECK(ofx_packed_pool_pairs(0, 22, 5000, &low, &high) == 20000);            // the default never drops below 4 * words
  CHECK(ofx_packed_pool_pairs(20000, 22, 5000, &low, &high) == 20000);
  CHECK(ofx_packed_pool_pairs(19999, 22, 5000, &low, &high) == 0);
  CHECK(ofx_packed_pool_pairs(((int64_t)1 << 31) - 1, 22, 5000, &low, &high) == ((int64_t)1 << 31) - 1);
  CHECK(ofx_packed_pool_pairs((int64_t)1 << 31, 22, 5000, &low, &high) == 0);
  CHECK(ofx_packed_pool_pairs(0, 0x7FFFFFFF, 5000, &low, &high) == 0);        // 512 * frames past 2^31
  CHECK(ofx_packed_store_bytes(4096, 502, 512 * 502) == 4096 * ((int64_t)512 * 502 * 8 + 502 * 12 + 16));

  // two arenas, F = 4.  Arena 0: the ring has wrapped, frame_head = 2, slots (tick): 0 (4), 1 (5), 2 (2), 3 (3) -
  // chronological order 2, 3, 0, 1.  Arena 1: slot 1 evicted early, frame_head = 0.
  Chunk c{2, 4, {4, 5, 2, 3, 7, -1, 9, 10}, {2, 0}, {3, 1, 0, 0, 5, 5, 2, 0, /* arena 1 */ 6, 0, 0, 0, 1, 1, 0, 9}};
  std::vector<uint32_t> off, ph, live;
  int64_t need = -1;
  CHECK(place(c, 100, off, ph, live, &need) == -1);
  CHECK(off[2] == 0 && off[3] == 10 && off[0] == 12 && off[1] == 16 && live[0] == 16 && ph[0] == 16);
  CHECK(off[4] == 0 && off[5] == 0 && off[6] == 6 && off[7] == 8 && live[1] == 17 && ph[1] == 17);
  // a pool that holds arena 0 exactly: pool_head wraps to 0; arena 1 needs one pair more and is refused
  CHECK(place(c, 16, off, ph, live, &need) == 1 && need == 17);
  CHECK(live[0] == 16 && ph[0] == 0 && live[1] == 0xDEADu);
  CHECK(place(c, 17, off, ph, live, &need) == -1 && ph[1] == 0 && ph[0] == 16);
  CHECK(place(c, 15, off, ph, live, &need) == 0 && need == 16);
  // counts at the top of their range, a pool near 2^31: no 32-bit overflow on the way
  Chunk big{1, 3, {0, 1, 2}, {0}, {0x3FFFFFFFu, 0x3FFFFFFFu, 0x3FFFFFFFu, 0x3FFFFFFFu, 5, 0}};
  CHECK(place(big, ((int64_t)1 << 31) - 1, off, ph, live, &need) == 0 && need == 4 * (int64_t)0x3FFFFFFF + 5);
  // an empty memory
  Chunk e{1, 2, {-1, -1}, {1}, {0, 0, 0, 0}};
  CHECK(place(e, 64, off, ph, live, &need) == -1 && live[0] == 0 && ph[0] == 0 && off[0] == 0 && off[1] == 0);
  printf("packed_place_check ok\n");
  return 0;
}
