// ofx_arena.h - the bump allocator every hand-carved device workspace of libofx.so is laid out with (plain C++17, no
// HIP: a host program can include it - tests/arena_host.cpp).  A workspace is ONE layout function that names its
// buffers and their counts; the caller runs it twice: on a measuring arena (no base: it only counts) to learn the bytes,
// then, the block ensured, on the block itself, and checks ok() once before the first launch.
#pragma once
#include <stddef.h>
#include <stdint.h>

struct Arena {
  char *base = nullptr;   // null: measuring, every request returns null
  size_t used = 0, cap = 0;
  bool over = false;
  Arena() {}
  Arena(void *block, size_t bytes) : base((char *)block), cap(bytes) {}
  // every request is rounded up to 256 bytes; one of 0 bytes advances nothing and gets the running position.  A request
  // past the block and every one after it get null (never memory of another buffer): ok() tells.
  void *take(size_t bytes) {
    const size_t step = (bytes + 255) & ~(size_t)255;
    if (!base) { used += step; return nullptr; }
    if (over || step > cap - used) { over = true; return nullptr; }
    char *p = base + used;
    used += step;
    return p;
  }
  template <class T> T *n(size_t count) { return (T *)take(count * sizeof(T)); }
  float *f(size_t count) { return n<float>(count); }
  double *d(size_t count) { return n<double>(count); }
  bool ok() const { return !over; }
};
