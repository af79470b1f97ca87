// api_sweep.hip -- sphere sweep queries (sweepkernel.hip, pt_sweep.h): the moptix_query_sweeps* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "sweepkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(moptix_sweep_hit) == sizeof(SweepHit), "moptix_sweep_hit is the kernel's record");
static_assert(MOPTIX_SWEEP_CLOSEST == SWEEP_CLOSEST && MOPTIX_SWEEP_ANY == SWEEP_ANY, "sweep query modes");

namespace {

size_t out_bytes(int32_t mode) { return mode == MOPTIX_SWEEP_ANY ? sizeof(int32_t) : sizeof(moptix_sweep_hit); }

int check_sweeps(moptix_context c, const float* sweeps, int64_t n, int32_t mode, const void* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_SWEEP_CLOSEST && mode != MOPTIX_SWEEP_ANY)) return fail(c, MOPTIX_ERR_INVALID, "bad sweep count or query mode");
  if (n > 0 && (!sweeps || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kSweepMaxLaunch sweeps.  The stack overflow area is the sweep
// queries' own: allocated at the first sweep query after a build, reused by every later one.
int enqueue_sweeps(moptix_context c, const float* dSweeps, int64_t n, int32_t mode, void* dOut) {
  SweepArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? sweepkernel_overflow_entries(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->sweep.overflow.ensure(ovf), "alloc sweep query stack overflow area");
    a.stackOverflow = c->sweep.overflow.p;
  }
  for (int64_t first = 0; first < n; first += kSweepMaxLaunch) {
    a.sweeps = dSweeps + 8 * first;
    a.out = static_cast<char*>(dOut) + out_bytes(mode) * (size_t)first;
    a.n = (int)(n - first < kSweepMaxLaunch ? n - first : kSweepMaxLaunch);
    HIPCHK(c, launch_sweepquery(c->stream, a, nBlocks, mode), "launch sweep query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_sweeps_device(moptix_context c, const float* dSweeps, int64_t n, int32_t mode, void* dOut) {
  int rc = check_sweeps(c, dSweeps, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dSweeps) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dOut) & (mode == MOPTIX_SWEEP_ANY ? 3u : 15u)) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "sweep queries read sweeps and write records 16 bytes at a time: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_sweeps(c, dSweeps, n, mode, dOut);
}

int moptix_query_sweeps(moptix_context c, const float* sweeps, int64_t n, int32_t mode, void* out) {
  int rc = check_sweeps(c, sweeps, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t bytes = out_bytes(mode) * (size_t)n;
  HIPCHK(c, c->sweep.sweeps.ensure(8 * (size_t)n), "alloc query sweeps");
  HIPCHK(c, c->sweep.out.ensure(bytes), "alloc sweep query results");
  HIPCHK(c, hipMemcpyAsync(c->sweep.sweeps.p, sweeps, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query sweeps");
  if ((rc = enqueue_sweeps(c, c->sweep.sweeps.p, n, mode, c->sweep.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->sweep.out.p, bytes } }, "read sweep query results");
}

}  // extern "C"
