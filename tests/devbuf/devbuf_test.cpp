// Ownership of DevBuf (csrc/devbuf.h) against counting fakes of the HIP calls (hip/hip_runtime.h next
// to this file).  Built with -fsanitize=address,undefined by tests/test_devbuf.py; never loaded into
// Python and never run on a GPU.  Exit status 0: every check held and allocations equal frees.
#include "devbuf.h"

#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
      ++failures;                                                 \
    }                                                             \
  } while (0)

// as the engine's groups: a struct of buffers, dropped by assigning a fresh one
struct Group {
  DevBuf<double> a, b;
  DevBuf<uint8_t> c;
};
struct Block : Group {
  int d = 0;
  DevBuf<int32_t> keep;  // not of the group: outlives its reset
};

int main() {
  FakeHip& f = fake_hip();
  {
    DevBuf<double> x;
    CHECK(!x && x.get() == nullptr);
    CHECK(x.alloc(0) == hipSuccess);  // zero elements: one, so a buffer in use is never null
    CHECK(x && f.last_bytes == sizeof(double));
    CHECK(x.alloc(10) == hipSuccess);  // re-alloc frees what was held
    CHECK(f.mallocs == 2 && f.frees == 1 && f.last_bytes == 10 * sizeof(double));
    CHECK(x.zero(10) == hipSuccess && x.get()[9] == 0.0);
    DevBuf<int64_t> t;
    CHECK(t.alloc(3) == hipSuccess && t.fill_bytes(0xff, 3) == hipSuccess && t.get()[2] == -1);
    CHECK(f.memsets == 2);

    double* raw = x;  // the implicit conversion the launch sites use
    DevBuf<double> y(std::move(x));  // move-construct: the source is left empty
    CHECK(!x && y.get() == raw && f.mallocs == 3 && f.frees == 1);

    DevBuf<double> z;
    CHECK(z.alloc(4) == hipSuccess);
    z = std::move(y);  // move-assign over a live buffer: the old one is freed, once
    CHECK(z.get() == raw && !y && f.frees == 2);
    DevBuf<double>& zr = z;
    z = std::move(zr);  // self-move keeps the buffer
    CHECK(z.get() == raw && f.frees == 2);

    z.reset();
    z.reset();  // idempotent
    CHECK(!z && f.frees == 3);

    f.fail_next = true;  // a failed allocation leaves the buffer empty, nothing to free later
    CHECK(z.alloc(8) == hipErrorOutOfMemory && !z);
    CHECK(z.alloc(8) == hipSuccess && z);
  }  // z and t go out of scope
  CHECK(f.mallocs == 5 && f.frees == 5);

  {  // pinned host memory goes back through hipHostFree
    DevBuf<int32_t, true> h;
    CHECK(h.alloc(8) == hipSuccess && h.zero(8) == hipSuccess && h.get()[7] == 0);
  }
  CHECK(f.host_mallocs == 1 && f.host_frees == 1 && f.mallocs == 5 && f.frees == 5);

  {  // a growing vector of structs that hold buffers moves them, never copies or frees them
    std::vector<Block> v;
    for (int i = 0; i < 9; ++i) {
      Block b;
      b.d = i;
      CHECK(b.a.alloc(i + 1) == hipSuccess && b.c.alloc(1) == hipSuccess && b.keep.alloc(2) == hipSuccess);
      b.a.get()[i] = (double)i;
      v.push_back(std::move(b));
    }
    CHECK(f.mallocs == 5 + 27 && f.frees == 5);
    for (int i = 0; i < 9; ++i) CHECK(v[i].d == i && v[i].a.get()[i] == (double)i && !v[i].b);
    // the group reset of free_dev: the group's buffers go, the rest of the struct stays
    for (Block& b : v) static_cast<Group&>(b) = Group();
    CHECK(f.frees == 5 + 18);
    for (int i = 0; i < 9; ++i) CHECK(!v[i].a && !v[i].c && v[i].keep && v[i].d == i);
    CHECK(v[3].a.alloc(5) == hipSuccess);  // and can be allocated again
  }
  CHECK(f.mallocs == f.frees && f.host_mallocs == f.host_frees);
  printf("devbuf: %ld allocations, %ld frees, %d failed checks\n", f.mallocs + f.host_mallocs,
         f.frees + f.host_frees, failures);
  return failures || f.mallocs != f.frees || f.host_mallocs != f.host_frees;
}
