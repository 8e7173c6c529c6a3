/* Host-side check of gpk_dev, the owner of the composite entries' device buffers (csrc/gpk_compose.h), on the CPU and
 * without a GPU: the four HIP calls it makes are replaced - in this program only - by a malloc / free / memset shim, so
 * that the host sanitizers see every allocation the owner makes, keeps and frees.  Stand-alone, not run through Python:
 *   hipcc -std=c++17 -Xarch_host -fsanitize=address,undefined tests/c_abi/gpk_dev_host.cpp -o gpk_dev_host && ./gpk_dev_host
 * Expected: "gpk_dev: ok", no sanitizer report, exit status 0 (a leak ends the program with LeakSanitizer's report). */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int live = 0, fills = 0, syncs = 0, fail_in = -1;   /* fail_in == 0: the next allocation fails */
static size_t last_fill = 0;

static hipError_t shim_malloc(void** p, size_t n) {
  if (fail_in == 0) return hipErrorOutOfMemory;
  if (fail_in > 0) --fail_in;
  *p = malloc(n);
  ++live;
  return hipSuccess;
}
static hipError_t shim_free(void* p) {
  free(p);
  --live;
  return hipSuccess;
}
static hipError_t shim_memset(void* p, int v, size_t n, hipStream_t) {
  memset(p, v, n);      /* (a fill beyond the block is the sanitizer's to report) */
  ++fills;
  last_fill = n;
  return hipSuccess;
}
static hipError_t shim_sync(hipStream_t) {
  ++syncs;
  return hipSuccess;
}
#define hipMalloc shim_malloc
#define hipFree shim_free
#define hipMemsetAsync shim_memset
#define hipStreamSynchronize shim_sync
#define hipGetErrorString(e) "shim: out of memory"
#include "../../unmanned_aerial_vehicles_amd/csrc/gpk_compose.h"

#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      fprintf(stderr, "gpk_dev_host.cpp:%d: %s\n", __LINE__, #cond);         \
      return 1;                                                              \
    }                                                                        \
  } while (0)

struct Model {      /* as gpk_model: freeing it is `delete` */
  gpk_dev<double> X, K;
  gpk_dev<void> q;
  gpk_lml_scratch trial;
};

/* three temporaries, the third allocation fails: the early return frees the first two */
static int early_return(gpk_handle h) {
  gpk_dev<double> a, b, c;
  GPK_TRY(a.alloc(h, 10));
  GPK_TRY(b.alloc(h, 20));
  fail_in = 0;
  GPK_TRY(c.alloc(h, 30));
  return GPK_OK;
}

static int run(gpk_handle h) {
  for (int fill = 0; fill < 2; ++fill) {
    h->debug_fill = fill;
    fills = 0;
    {
      gpk_dev<double> a;
      EXPECT(!a && a.bytes == 0);
      EXPECT(a.alloc(h, 100) == GPK_OK && a.p && a.bytes == 800 && live == 1 && fills == fill && (!fill || last_fill == 800));
      a[99] = 1.0;
      EXPECT(a.alloc(h, 7) == GPK_OK && a.bytes == 56 && live == 1);      /* again: the first block is freed */
      a.reset();
      EXPECT(!a && a.bytes == 0 && live == 0);
      a.reset();                                                           /* twice: nothing to free */
      EXPECT(live == 0);
    }
    {
      gpk_dev<void> q;
      const int s0 = syncs, f0 = fills;
      EXPECT(q.reserve(h, 0) == GPK_OK && !q && live == 0 && syncs == s0 && fills == f0);
      EXPECT(q.reserve(h, 256) == GPK_OK && q.bytes == 256 && live == 1 && syncs == s0 + 1);             /* grows */
      void* first = q;
      EXPECT(q.reserve(h, 64) == GPK_OK && q.p == first && q.bytes == 256 && syncs == s0 + 1);             /* does not */
      EXPECT(fills == f0 + 2 * fill && (!fill || last_fill == 64));      /* ... and is filled at every request, as asked for */
      EXPECT(q.reserve(h, 4096) == GPK_OK && q.bytes == 4096 && live == 1 && syncs == s0 + 2);           /* grows again */
      ((char*)q.p)[4095] = 1;
      fail_in = 0;                                                         /* a failed growth leaves an empty, reusable owner */
      EXPECT(q.reserve(h, 8192) == GPK_HIP_ERROR && !q && q.bytes == 0 && live == 0);
      fail_in = -1;
      EXPECT(q.reserve(h, 16) == GPK_OK && q.bytes == 16 && live == 1);
    }
    EXPECT(live == 0);      /* destruction */
    EXPECT(early_return(h) == GPK_HIP_ERROR && live == 0 && h->err.find("hipMalloc") != std::string::npos);
    fail_in = -1;
    {
      Model* m = new Model();
      EXPECT(m->X.alloc(h, 6) == GPK_OK && m->K.alloc(h, 16) == GPK_OK && m->q.reserve(h, 100) == GPK_OK);
      fail_in = 2;          /* the scratch of the trial evaluations fails at its third block ... */
      EXPECT(m->trial.ensure(h, 16, 9, 8, 4, true) == GPK_HIP_ERROR && live == 5);
      fail_in = -1;         /* ... and is taken up again whole */
      EXPECT(m->trial.ensure(h, 16, 9, 8, 4, false) == GPK_OK && live == 8 && !m->trial.Kinv);
      EXPECT(m->trial.ensure(h, 16, 9, 8, 4, true) == GPK_OK && live == 9);
      m->trial.alpha[3] = m->trial.Kinv[15] = 0.0;
      delete m;
      EXPECT(live == 0);
    }
  }
  return 0;
}

int main() {
  gpk_context ctx;
  if (run(&ctx) != 0) return 1;
  printf("gpk_dev: ok\n");
  return 0;
}
