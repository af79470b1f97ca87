// api_tri.hip -- triangle queries (trikernel.hip, pt_tri.h): the moptix_query_tris* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "trikernel.h"

using namespace pt;
using namespace pt::api;

static_assert(MOPTIX_BOX_ANY == BOX_ANY && MOPTIX_BOX_COUNT == BOX_COUNT, "box query modes");
static_assert(sizeof(long long) == sizeof(int64_t), "the kernel reads the offsets as long long");

namespace {

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_tris(moptix_context c, const float* tris, int64_t n, int32_t mode, const int32_t* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_BOX_ANY && mode != MOPTIX_BOX_COUNT)) return fail(c, MOPTIX_ERR_INVALID, "bad triangle count or query mode");
  if (n > 0 && (!tris || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

int check_tris_list(moptix_context c, const float* tris, int64_t n, const int64_t* offsets, const int32_t* prims, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0) return fail(c, MOPTIX_ERR_INVALID, "bad triangle count");
  if (n > 0 && (!tris || !offsets || !prims || !counts)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kTriMaxLaunch queries.  The stack overflow area is the triangle
// queries' own: allocated at the first such query after a build, reused by every later one.  mode BOX_LIST: dOut takes the counts.
int enqueue_tris(moptix_context c, const float* dTris, int64_t n, int mode, int32_t* dOut, const int64_t* dOffsets, int32_t* dPrims) {
  TriArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? trikernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->tri.overflow.ensure(ovf), "alloc triangle query stack overflow area");
    a.stackOverflow = c->tri.overflow.p;
  }
  a.prims = dPrims;
  for (int64_t first = 0; first < n; first += kTriMaxLaunch) {
    a.tris = dTris + 9 * first;
    a.out = dOut + first;
    a.offsets = dOffsets ? reinterpret_cast<const long long*>(dOffsets) + first : nullptr;
    a.n = (int)(n - first < kTriMaxLaunch ? n - first : kTriMaxLaunch);
    HIPCHK(c, launch_triquery(c->stream, a, nBlocks, mode), mode == BOX_LIST ? "launch triangle list query" : "launch triangle query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_tris_device(moptix_context c, const float* dTris, int64_t n, int32_t mode, int32_t* dOut) {
  int rc = check_tris(c, dTris, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dTris, 3u) || misaligned(dOut, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "triangle queries read float32 vertices and write int32 results: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_tris(c, dTris, n, mode, dOut, nullptr, nullptr);
}

int moptix_query_tris(moptix_context c, const float* tris, int64_t n, int32_t mode, int32_t* out) {
  int rc = check_tris(c, tris, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  HIPCHK(c, c->tri.tris.ensure(9 * (size_t)n), "alloc query triangles");
  HIPCHK(c, c->tri.out.ensure((size_t)n), "alloc triangle query results");
  HIPCHK(c, hipMemcpyAsync(c->tri.tris.p, tris, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query triangles");
  if ((rc = enqueue_tris(c, c->tri.tris.p, n, mode, c->tri.out.p, nullptr, nullptr)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->tri.out.p, sizeof(int32_t) * (size_t)n } }, "read triangle query results");
}

int moptix_query_tris_list_device(moptix_context c, const float* dTris, int64_t n, const int64_t* dOffsets, int32_t* dPrims, int32_t* dCounts) {
  int rc = check_tris_list(c, dTris, n, dOffsets, dPrims, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dTris, 3u) || misaligned(dOffsets, 7u) || misaligned(dPrims, 3u) || misaligned(dCounts, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "triangle list queries read float32 vertices, offsets 8 bytes at a time and write int32 ids and counts: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_tris(c, dTris, n, BOX_LIST, dCounts, dOffsets, dPrims);
}

int moptix_query_tris_list(moptix_context c, const float* tris, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  int rc = check_tris_list(c, tris, n, offsets, prims, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (offsets[0] < 0) return fail(c, MOPTIX_ERR_INVALID, "offsets[0] must be >= 0");
  for (int64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, MOPTIX_ERR_INVALID, "offsets must not decrease");
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  // the staging of prims covers 0 .. offsets[n], so that the caller's offsets serve as they are; the slices' span is read back
  const size_t lo = (size_t)offsets[0], hi = (size_t)offsets[n];
  HIPCHK(c, c->tri.tris.ensure(9 * (size_t)n), "alloc query triangles");
  HIPCHK(c, c->tri.offsets.ensure((size_t)n + 1), "alloc triangle list offsets");
  HIPCHK(c, c->tri.prims.ensure(hi), "alloc triangle list ids");
  HIPCHK(c, c->tri.out.ensure((size_t)n), "alloc triangle query results");
  HIPCHK(c, hipMemcpyAsync(c->tri.tris.p, tris, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query triangles");
  HIPCHK(c, hipMemcpyAsync(c->tri.offsets.p, offsets, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream), "upload triangle list offsets");
  if ((rc = enqueue_tris(c, c->tri.tris.p, n, BOX_LIST, c->tri.out.p, reinterpret_cast<const int64_t*>(c->tri.offsets.p), c->tri.prims.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { hi > lo ? prims + lo : nullptr, c->tri.prims.p + lo, sizeof(int32_t) * (hi - lo) }, { counts, c->tri.out.p, sizeof(int32_t) * (size_t)n } },
                   "read triangle list results");
}

}  // extern "C"
