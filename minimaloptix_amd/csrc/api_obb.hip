// api_obb.hip -- oriented box queries (obbkernel.hip, pt_obb.h): the moptix_query_obbs* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "obbkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(MOPTIX_BOX_ANY == BOX_ANY && MOPTIX_BOX_COUNT == BOX_COUNT, "box query modes");
static_assert(sizeof(long long) == sizeof(int64_t), "the kernel reads the offsets as long long");

namespace {

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_obbs(moptix_context c, const float* obbs, int64_t n, int32_t mode, const int32_t* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_BOX_ANY && mode != MOPTIX_BOX_COUNT)) return fail(c, MOPTIX_ERR_INVALID, "bad oriented box count or query mode");
  if (n > 0 && (!obbs || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

int check_obbs_list(moptix_context c, const float* obbs, int64_t n, const int64_t* offsets, const int32_t* prims, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0) return fail(c, MOPTIX_ERR_INVALID, "bad oriented box count");
  if (n > 0 && (!obbs || !offsets || !prims || !counts)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kObbMaxLaunch boxes.  The stack overflow area is the oriented box
// queries' own: allocated at the first such query after a build, reused by every later one.  mode BOX_LIST: dOut takes the counts.
int enqueue_obbs(moptix_context c, const float* dObbs, int64_t n, int mode, int32_t* dOut, const int64_t* dOffsets, int32_t* dPrims) {
  ObbArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? obbkernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->obb.overflow.ensure(ovf), "alloc oriented box query stack overflow area");
    a.stackOverflow = c->obb.overflow.p;
  }
  a.prims = dPrims;
  for (int64_t first = 0; first < n; first += kObbMaxLaunch) {
    a.obbs = dObbs + 16 * first;
    a.out = dOut + first;
    a.offsets = dOffsets ? reinterpret_cast<const long long*>(dOffsets) + first : nullptr;
    a.n = (int)(n - first < kObbMaxLaunch ? n - first : kObbMaxLaunch);
    HIPCHK(c, launch_obbquery(c->stream, a, nBlocks, mode), mode == BOX_LIST ? "launch oriented box list query" : "launch oriented box query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_obbs_device(moptix_context c, const float* dObbs, int64_t n, int32_t mode, int32_t* dOut) {
  int rc = check_obbs(c, dObbs, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dObbs, 15u) || misaligned(dOut, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "oriented box queries read boxes 16 bytes at a time and write int32 results: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_obbs(c, dObbs, n, mode, dOut, nullptr, nullptr);
}

int moptix_query_obbs(moptix_context c, const float* obbs, int64_t n, int32_t mode, int32_t* out) {
  int rc = check_obbs(c, obbs, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  HIPCHK(c, c->obb.obbs.ensure(16 * (size_t)n), "alloc query oriented boxes");
  HIPCHK(c, c->obb.out.ensure((size_t)n), "alloc oriented box query results");
  HIPCHK(c, hipMemcpyAsync(c->obb.obbs.p, obbs, sizeof(float) * 16 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query oriented boxes");
  if ((rc = enqueue_obbs(c, c->obb.obbs.p, n, mode, c->obb.out.p, nullptr, nullptr)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->obb.out.p, sizeof(int32_t) * (size_t)n } }, "read oriented box query results");
}

int moptix_query_obbs_list_device(moptix_context c, const float* dObbs, int64_t n, const int64_t* dOffsets, int32_t* dPrims, int32_t* dCounts) {
  int rc = check_obbs_list(c, dObbs, n, dOffsets, dPrims, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dObbs, 15u) || misaligned(dOffsets, 7u) || misaligned(dPrims, 3u) || misaligned(dCounts, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "oriented box list queries read boxes 16 and offsets 8 bytes at a time and write int32 ids and counts: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_obbs(c, dObbs, n, BOX_LIST, dCounts, dOffsets, dPrims);
}

int moptix_query_obbs_list(moptix_context c, const float* obbs, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  int rc = check_obbs_list(c, obbs, n, offsets, prims, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (offsets[0] < 0) return fail(c, MOPTIX_ERR_INVALID, "offsets[0] must be >= 0");
  for (int64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, MOPTIX_ERR_INVALID, "offsets must not decrease");
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  // the staging of prims covers 0 .. offsets[n], so that the caller's offsets serve as they are; the slices' span is read back
  const size_t lo = (size_t)offsets[0], hi = (size_t)offsets[n];
  HIPCHK(c, c->obb.obbs.ensure(16 * (size_t)n), "alloc query oriented boxes");
  HIPCHK(c, c->obb.offsets.ensure((size_t)n + 1), "alloc oriented box list offsets");
  HIPCHK(c, c->obb.prims.ensure(hi), "alloc oriented box list ids");
  HIPCHK(c, c->obb.out.ensure((size_t)n), "alloc oriented box query results");
  HIPCHK(c, hipMemcpyAsync(c->obb.obbs.p, obbs, sizeof(float) * 16 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query oriented boxes");
  HIPCHK(c, hipMemcpyAsync(c->obb.offsets.p, offsets, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream), "upload oriented box list offsets");
  if ((rc = enqueue_obbs(c, c->obb.obbs.p, n, BOX_LIST, c->obb.out.p, reinterpret_cast<const int64_t*>(c->obb.offsets.p), c->obb.prims.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { hi > lo ? prims + lo : nullptr, c->obb.prims.p + lo, sizeof(int32_t) * (hi - lo) }, { counts, c->obb.out.p, sizeof(int32_t) * (size_t)n } },
                   "read oriented box list results");
}

}  // extern "C"
