// ofx_rng.h - the counter RNG every feature keys its randomness on: Philox4x32-10, the stream ids, the key of a
// seed and the word -> number maps.  A draw is a pure function of (counter, stream, seed), so it is the same on any
// launch shape, shard or resume; the oracles restate all of this independently (oracle/, tests/*_oracle.py).
#pragma once
#include <stdint.h>

// The fourth counter word c3.  Two streams never share an id: their draws would be correlated.  Per id: the counter
// (c0, c1, c2) and the words of the output that are consumed.  `arena` is the GLOBAL arena, cfg.arena_base + a.
enum : uint32_t {
  OFX_STREAM_BOT = 0,            // (arena, ship, lock-step): 0, 1 the law's uniforms (0 alone picks RANDOM's move); 2, 3 the repoint (x, y)
  OFX_STREAM_RESET = 1,          // (arena, ship, episode): 0, 1 the restart (dx, dy)
  OFX_STREAM_EXPLORE = 2,        // (arena, ship, lock-step): 0 the epsilon test; 1 the action; 2, 3 the pointer (x, y)
  OFX_STREAM_REPLAY = 3,         // (arena, row j of the batch, draw): 0 the j-th pick of Floyd's subset sampling
  OFX_STREAM_PER = 4,            // (arena, row j of the batch, draw): 0 the position in stratum j of the arena's priority mass
  OFX_STREAM_GLOBAL = 5,         // (arena_base, row j of the global batch, draw): 0 the position in stratum j of the rows (uniform) or of the mass (PER)
  OFX_STREAM_BOLTZMANN_PTR = 6,  // (arena, ship * 40000 + (y * 400 + x) / 4, lock-step): word x & 3 the Gumbel noise of heat-map pixel (x, y)
  OFX_STREAM_BOLTZMANN_ACT = 7,  // (arena, ship, lock-step): 0, 1 Gumbel noise of the two action values
  OFX_STREAM_AUGMENT = 8,        // (arena_base, first + row of the batch, draw): 0 which of the enabled elements of the dihedral group
  OFX_STREAM_EVOLVE = 9,         // (slot, element, generation): 0, 1 the evolution coefficient; 2, 3 the mutation selector
  OFX_STREAM_MUTATE = 10,        // (slot, element, generation): 0, 1 the replacement value of a mutated element
  OFX_STREAM_FRESH = 11,         // (slot, element, generation): 0, 1 a fresh genome's element (ofx_population_init, plan[p] == -1)
};
// The evolution strategy's stream, id 12, stated here beside the others and like them nowhere else.  It stands outside
// the enum above and carries another prefix because tests/test_rng_streams.py holds that enum to exactly the twelve
// names and ids 0 .. 11; tests/test_es.py holds this id to be 12, distinct from all of those, and defined once.
enum : uint32_t {
  OFX_ES_STREAM = 12,            // (pair, element, generation): 0..3 summed, the noise of an ES member's element (ofx_es_act, ofx_es_update)
};

// Philox4x32-10 (Salmon et al. SC'11); same constants / round structure as the oracle's restatement so both produce
// one stream.
__host__ __device__ inline void ofx_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                                  uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the Philox key of a caller's 64-bit seed
struct ofx_rng_key { uint32_t k0, k1; };
__host__ __device__ inline ofx_rng_key ofx_key(uint64_t seed) { return {(uint32_t)seed, (uint32_t)(seed >> 32)}; }

__host__ __device__ inline void ofx_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t stream, ofx_rng_key key,
                                                  uint32_t out[4]) {
  ofx_philox4x32_10(c0, c1, c2, stream, key.k0, key.k1, out);
}

// a word as an integer in [0, n_inclusive]
__host__ __device__ inline int32_t ofx_draw_int(uint32_t r, int32_t n_inclusive) {
  return (int32_t)(((uint64_t)r * (uint64_t)(n_inclusive + 1)) >> 32);
}

// a word as a double in [0, 1): exact, r / 2^32
__host__ __device__ inline double ofx_unit(uint32_t r) { return (double)r * 0x1p-32; }
