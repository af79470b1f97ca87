// api_query.hip -- batched ray queries (querykernel.hip, pt_query.h, pt_multihit.h): the moptix_query_rays* and moptix_query_rays_multi*
// entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "pt_multihit.h"
#include "pt_query.h"
#include "querykernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(moptix_hit) == sizeof(QueryHit), "moptix_hit is the kernel's record");
static_assert(MOPTIX_QUERY_CLOSEST == QUERY_CLOSEST && MOPTIX_QUERY_ANY == QUERY_ANY, "query modes");
static_assert(MOPTIX_MULTI_COUNT_ALL == MULTI_COUNT_ALL, "multi-hit flags");

namespace {

size_t out_bytes(int32_t mode) { return mode == MOPTIX_QUERY_ANY ? sizeof(int32_t) : sizeof(moptix_hit); }

int check_query(moptix_context c, const float* rays, int64_t n, int32_t mode, void* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_QUERY_CLOSEST && mode != MOPTIX_QUERY_ANY)) return fail(c, MOPTIX_ERR_INVALID, "bad ray count or query mode");
  if (n > 0 && (!rays || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kQueryMaxLaunch rays.  The stack overflow area is the context's:
// allocated at the first query after a build, reused by every later one.
int enqueue_query(moptix_context c, const float* dRays, int64_t n, int32_t mode, void* dOut) {
  QueryArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? querykernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->query.overflow.ensure(ovf), "alloc query stack overflow area");
    a.stackOverflow = c->query.overflow.p;
  }
  for (int64_t first = 0; first < n; first += kQueryMaxLaunch) {
    a.rays = dRays + 8 * first;
    a.out = static_cast<char*>(dOut) + out_bytes(mode) * (size_t)first;
    a.n = (int)(n - first < kQueryMaxLaunch ? n - first : kQueryMaxLaunch);
    HIPCHK(c, launch_rayquery(c->stream, a, nBlocks, mode), "launch ray query");
  }
  return MOPTIX_OK;
}

int check_multi(moptix_context c, const float* rays, int64_t n, int32_t maxHits, uint32_t flags, const void* hits, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (flags & ~(uint32_t)MOPTIX_MULTI_COUNT_ALL) != 0) return fail(c, MOPTIX_ERR_INVALID, "bad ray count or unknown multi-hit flag");
  const int lowest = (flags & MOPTIX_MULTI_COUNT_ALL) ? 0 : 1;
  if (maxHits < lowest || maxHits > kMultiMaxHits) return fail(c, MOPTIX_ERR_INVALID, "maxHits out of range (1..64; 0 only with MOPTIX_MULTI_COUNT_ALL)");
  if (n > 0 && (!rays || !counts || (maxHits > 0 && !hits))) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// As enqueue_query, with the ray queries' overflow area.  A launch takes at most kQueryMaxLaunch / max(maxHits, 1) rays, so that the
// index of a record within a launch fits 32 bits as the index of a ray does.
int enqueue_multi(moptix_context c, const float* dRays, int64_t n, int32_t maxHits, uint32_t flags, void* dHits, int32_t* dCounts) {
  MultiArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? querykernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->query.overflow.ensure(ovf), "alloc query stack overflow area");
    a.stackOverflow = c->query.overflow.p;
  }
  a.maxHits = maxHits;
  const int64_t perLaunch = kQueryMaxLaunch / (maxHits > 0 ? maxHits : 1);
  for (int64_t first = 0; first < n; first += perLaunch) {
    a.rays = dRays + 8 * first;
    a.hits = maxHits > 0 ? static_cast<char*>(dHits) + sizeof(moptix_hit) * (size_t)maxHits * (size_t)first : nullptr;
    a.counts = dCounts + first;
    a.n = (int)(n - first < perLaunch ? n - first : perLaunch);
    HIPCHK(c, launch_rayquery_multi(c->stream, a, nBlocks, (flags & MOPTIX_MULTI_COUNT_ALL) != 0), "launch multi-hit ray query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_rays_device(moptix_context c, const float* dRays, int64_t n, int32_t mode, void* dOut) {
  int rc = check_query(c, dRays, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dRays) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dOut) & (mode == MOPTIX_QUERY_ANY ? 3u : 15u)) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "ray queries read rays and write hit records 16 bytes at a time: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_query(c, dRays, n, mode, dOut);
}

int moptix_query_rays(moptix_context c, const float* rays, int64_t n, int32_t mode, void* out) {
  int rc = check_query(c, rays, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t bytes = out_bytes(mode) * (size_t)n;
  HIPCHK(c, c->query.rays.ensure(8 * (size_t)n), "alloc query rays");
  HIPCHK(c, c->query.out.ensure(bytes), "alloc query results");
  HIPCHK(c, hipMemcpyAsync(c->query.rays.p, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query rays");
  if ((rc = enqueue_query(c, c->query.rays.p, n, mode, c->query.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->query.out.p, bytes } }, "read query results");
}

int moptix_query_rays_multi_device(moptix_context c, const float* dRays, int64_t n, int32_t maxHits, uint32_t flags, void* dHits, int32_t* dCounts) {
  int rc = check_multi(c, dRays, n, maxHits, flags, dHits, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dRays) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dHits) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dCounts) & 3u) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "multi-hit queries read rays and write hit records 16 bytes at a time, counts 4: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_multi(c, dRays, n, maxHits, flags, dHits, dCounts);
}

int moptix_query_rays_multi(moptix_context c, const float* rays, int64_t n, int32_t maxHits, uint32_t flags, moptix_hit* hits, int32_t* counts) {
  int rc = check_multi(c, rays, n, maxHits, flags, hits, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t hitBytes = sizeof(moptix_hit) * (size_t)maxHits * (size_t)n, countBytes = sizeof(int32_t) * (size_t)n;      // counts behind the records
  HIPCHK(c, c->query.rays.ensure(8 * (size_t)n), "alloc query rays");
  HIPCHK(c, c->query.out.ensure(hitBytes + countBytes), "alloc query results");
  HIPCHK(c, hipMemcpyAsync(c->query.rays.p, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query rays");
  int32_t* dCounts = reinterpret_cast<int32_t*>(c->query.out.p + hitBytes);
  if ((rc = enqueue_multi(c, c->query.rays.p, n, maxHits, flags, c->query.out.p, dCounts)) != MOPTIX_OK) return rc;
  return read_back(c, { { maxHits > 0 ? hits : nullptr, c->query.out.p, hitBytes }, { counts, dCounts, countBytes } }, "read multi-hit results");
}

}  // extern "C"
