// api_frustum.hip --frustum queries (frustumkernel.hip, pt_frustum.h): the moptix_query_frusta* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "frustumkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(MOPTIX_BOX_ANY == BOX_ANY && MOPTIX_BOX_COUNT == BOX_COUNT, "box query modes");
static_assert(sizeof(long long) == sizeof(int64_t), "the kernel reads the offsets as long long");

namespace {

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_frusta(moptix_context c, const float* frusta, int64_t n, int32_t mode, const int32_t* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_BOX_ANY && mode != MOPTIX_BOX_COUNT)) return fail(c, MOPTIX_ERR_INVALID, "bad frustum count or query mode");
  if (n > 0 && (!frusta || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

int check_frusta_list(moptix_context c, const float* frusta, int64_t n, const int64_t* offsets, const int32_t* prims, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0) return fail(c, MOPTIX_ERR_INVALID, "bad frustum count");
  if (n > 0 && (!frusta || !offsets || !prims || !counts)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kFrustumMaxLaunch queries.  The stack overflow area is the frustum
// queries' own: allocated at the first such query after a build, reused by every later one.  mode BOX_LIST: dOut takes the counts.
int enqueue_frusta(moptix_context c, const float* dFrusta, int64_t n, int mode, int32_t* dOut, const int64_t* dOffsets, int32_t* dPrims) {
  FrustumArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? frustumkernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->frustum.overflow.ensure(ovf), "alloc frustum query stack overflow area");
    a.stackOverflow = c->frustum.overflow.p;
  }
  a.prims = dPrims;
  for (int64_t first = 0; first < n; first += kFrustumMaxLaunch) {
    a.frusta = dFrusta + 24 * first;
    a.out = dOut + first;
    a.offsets = dOffsets ? reinterpret_cast<const long long*>(dOffsets) + first : nullptr;
    a.n = (int)(n - first < kFrustumMaxLaunch ? n - first : kFrustumMaxLaunch);
    HIPCHK(c, launch_frustumquery(c->stream, a, nBlocks, mode), mode == BOX_LIST ? "launch frustum list query" : "launch frustum query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_frusta_device(moptix_context c, const float* dFrusta, int64_t n, int32_t mode, int32_t* dOut) {
  int rc = check_frusta(c, dFrusta, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dFrusta, 15u) || misaligned(dOut, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "frustum queries read planes 16 bytes at a time and write int32 results: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_frusta(c, dFrusta, n, mode, dOut, nullptr, nullptr);
}

int moptix_query_frusta(moptix_context c, const float* frusta, int64_t n, int32_t mode, int32_t* out) {
  int rc = check_frusta(c, frusta, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  HIPCHK(c, c->frustum.frusta.ensure(24 * (size_t)n), "alloc query frusta");
  HIPCHK(c, c->frustum.out.ensure((size_t)n), "alloc frustum query results");
  HIPCHK(c, hipMemcpyAsync(c->frustum.frusta.p, frusta, sizeof(float) * 24 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query frusta");
  if ((rc = enqueue_frusta(c, c->frustum.frusta.p, n, mode, c->frustum.out.p, nullptr, nullptr)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->frustum.out.p, sizeof(int32_t) * (size_t)n } }, "read frustum query results");
}

int moptix_query_frusta_list_device(moptix_context c, const float* dFrusta, int64_t n, const int64_t* dOffsets, int32_t* dPrims, int32_t* dCounts) {
  int rc = check_frusta_list(c, dFrusta, n, dOffsets, dPrims, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dFrusta, 15u) || misaligned(dOffsets, 7u) || misaligned(dPrims, 3u) || misaligned(dCounts, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "frustum list queries read planes 16 and offsets 8 bytes at a time and write int32 ids and counts: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_frusta(c, dFrusta, n, BOX_LIST, dCounts, dOffsets, dPrims);
}

int moptix_query_frusta_list(moptix_context c, const float* frusta, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  int rc = check_frusta_list(c, frusta, n, offsets, prims, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (offsets[0] < 0) return fail(c, MOPTIX_ERR_INVALID, "offsets[0] must be >= 0");
  for (int64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, MOPTIX_ERR_INVALID, "offsets must not decrease");
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  // the staging of prims covers 0 .. offsets[n], so that the caller's offsets serve as they are; the slices' span is read back
  const size_t lo = (size_t)offsets[0], hi = (size_t)offsets[n];
  HIPCHK(c, c->frustum.frusta.ensure(24 * (size_t)n), "alloc query frusta");
  HIPCHK(c, c->frustum.offsets.ensure((size_t)n + 1), "alloc frustum list offsets");
  HIPCHK(c, c->frustum.prims.ensure(hi), "alloc frustum list ids");
  HIPCHK(c, c->frustum.out.ensure((size_t)n), "alloc frustum query results");
  HIPCHK(c, hipMemcpyAsync(c->frustum.frusta.p, frusta, sizeof(float) * 24 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query frusta");
  HIPCHK(c, hipMemcpyAsync(c->frustum.offsets.p, offsets, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream), "upload frustum list offsets");
  if ((rc = enqueue_frusta(c, c->frustum.frusta.p, n, BOX_LIST, c->frustum.out.p, reinterpret_cast<const int64_t*>(c->frustum.offsets.p), c->frustum.prims.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { hi > lo ? prims + lo : nullptr, c->frustum.prims.p + lo, sizeof(int32_t) * (hi - lo) }, { counts, c->frustum.out.p, sizeof(int32_t) * (size_t)n } },
                   "read frustum list results");
}

}  // extern "C"
