// The workspace arena of libofx.so (ofighters_amd/csrc/ofx_arena.h) on the host, by itself: tests/test_arena_host.py
// compiles this file with the system C++ compiler, runs it and expects exit status 0.  Every failed check prints its line.
#include "ofx_arena.h"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

int main() {
  const std::vector<size_t> req = {0, 1, 255, 256, 257, 4 * 5008 * 100, 0, 8 * 33};
  size_t total = 0;
  for (size_t b : req) total += up256(b);

  // (a) measuring: no base, counts only; a request of 0 bytes adds nothing
  {
    Arena A;
    for (size_t b : req) {
      const size_t before = A.used;
      CHECK(A.take(b) == nullptr);
      CHECK(A.used == before + up256(b));
      if (b == 0) CHECK(A.used == before);
    }
    CHECK(A.used == total);
    CHECK(A.ok());
  }

  char *block = (char *)std::aligned_alloc(256, total);
  if (!block) { std::printf("no memory\n"); return 2; }

  // (b) handing out on a block of exactly the measured size: base + the prefix sums, all 256-aligned, ends at cap
  {
    Arena A(block, total);
    size_t at = 0;
    for (size_t b : req) {
      char *p = (char *)A.take(b);
      CHECK(p == block + at);                  // (a zero-size request: the running position)
      CHECK(((uintptr_t)p & 255) == 0);
      at += up256(b);
    }
    CHECK(A.used == total && A.used == A.cap);
    CHECK(A.ok());
  }

  // (c) a block that is too short - by 256 bytes (the last request fails) and down to 1024 bytes (the 257-byte request
  // fails; two more and a zero-size one follow it): nothing handed out reaches past the block, the failing request and
  // every later one get null, ok() tells
  for (size_t cap : {total - 256, (size_t)1024}) {
    Arena A(block, cap);
    size_t at = 0;
    bool failed = false;
    for (size_t b : req) {
      char *p = (char *)A.take(b);
      if (!failed && at + up256(b) > cap) failed = true;
      if (failed) CHECK(p == nullptr);
      else {
        CHECK(p == block + at);
        CHECK(p + b <= block + cap);
        at += up256(b);
      }
    }
    CHECK(failed);
    CHECK(!A.ok());
    CHECK(A.used <= cap);
  }

  // (d) the typed helpers: 4 n and 8 n bytes (64 floats / 32 doubles fill a 256-byte slot, one more takes the next)
  {
    Arena M;
    M.f(64); CHECK(M.used == 256);
    M.f(65); CHECK(M.used == 256 + 512);
    M.d(32); CHECK(M.used == 1024);
    M.d(33); CHECK(M.used == 1536);
    M.n<int32_t>(65); CHECK(M.used == 2048);
    M.n<uint8_t>(257); CHECK(M.used == 2560);
    M.n<unsigned long long>(33); CHECK(M.used == 3072);
    Arena A(block, 3072);
    float *f0 = A.f(64), *f1 = A.f(65);
    double *d0 = A.d(32), *d1 = A.d(33);
    int32_t *i0 = A.n<int32_t>(65);
    CHECK((char *)f1 - (char *)f0 == 4 * 64);
    CHECK((char *)d0 - (char *)f1 == 512);
    CHECK((char *)d1 - (char *)d0 == 8 * 32);
    CHECK((char *)i0 - (char *)d1 == 512);
    f1[64] = 1.f; d1[32] = 2.0; i0[64] = 3;     // the last element of each is inside its slot (a sanitizer build tells)
    CHECK(A.ok());
  }

  std::free(block);
  if (failures) std::printf("%d checks failed\n", failures);
  return failures ? 1 : 0;
}
