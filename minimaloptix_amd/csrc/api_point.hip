// api_point.hip -- closest-point queries (pointkernel.hip, pt_point.h): the moptix_query_points* entry points of include/moptix.h.
// The signed mode's table is api_sign.hip's (sign_table_for_query); everything else of the three modes is here, and the K-nearest
// queries' moptix_query_points_multi* pair (pt_pointmulti.h), which shares the overflow area and the staging.
#include <cstring>

#include "api_context.h"
#include "pt_pointmulti.h"
#include "pointkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(moptix_point_hit) == sizeof(PointHit), "moptix_point_hit is the kernel's record");
static_assert(MOPTIX_POINT_CLOSEST == POINT_CLOSEST && MOPTIX_POINT_ANY == POINT_ANY && MOPTIX_POINT_SIGNED == POINT_SIGNED, "point query modes");
static_assert(MOPTIX_POINT_MULTI_COUNT_ALL == POINT_MULTI_COUNT_ALL, "K-nearest flags");

namespace {

size_t out_bytes(int32_t mode) { return mode == MOPTIX_POINT_ANY ? sizeof(int32_t) : sizeof(moptix_point_hit); }

// withSigned: the entry takes MOPTIX_POINT_SIGNED.  moptix_query_points does not: its modes are the two it had (2 stays
// MOPTIX_ERR_INVALID there, as callers and tests of it have it); the host-pointer form of the signed mode is moptix_query_points_signed.
int check_points(moptix_context c, const float* points, int64_t n, int32_t mode, void* out, bool withSigned) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_POINT_CLOSEST && mode != MOPTIX_POINT_ANY && !(withSigned && mode == MOPTIX_POINT_SIGNED))) return fail(c, MOPTIX_ERR_INVALID, "bad point count or query mode");
  if (n > 0 && (!points || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kPointMaxLaunch points.  The stack overflow area is the point
// queries' own: allocated at the first point query after a build, reused by every later one.  The signed mode's table goes first: the
// topology, its upload and the table build are in front of the query kernel on the stream.
int enqueue_points(moptix_context c, const float* dPoints, int64_t n, int32_t mode, void* dOut) {
  const SignRecord* table = nullptr;
  if (mode == MOPTIX_POINT_SIGNED) {
    const int rc = sign_table_for_query(c, table);
    if (rc != MOPTIX_OK) return rc;
  }
  PointArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? pointkernel_overflow_entries(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->point.overflow.ensure(ovf), "alloc point query stack overflow area");
    a.stackOverflow = c->point.overflow.p;
  }
  for (int64_t first = 0; first < n; first += kPointMaxLaunch) {
    a.points = dPoints + 4 * first;
    a.out = static_cast<char*>(dOut) + out_bytes(mode) * (size_t)first;
    a.n = (int)(n - first < kPointMaxLaunch ? n - first : kPointMaxLaunch);
    HIPCHK(c, launch_pointquery(c->stream, a, table, nBlocks, mode), mode == MOPTIX_POINT_SIGNED ? "launch signed point query" : "launch point query");
  }
  return MOPTIX_OK;
}

int check_points_multi(moptix_context c, const float* points, int64_t n, int32_t maxNear, uint32_t flags, const void* hits, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (flags & ~(uint32_t)MOPTIX_POINT_MULTI_COUNT_ALL) != 0) return fail(c, MOPTIX_ERR_INVALID, "bad point count or unknown K-nearest flag");
  const int lowest = (flags & MOPTIX_POINT_MULTI_COUNT_ALL) ? 0 : 1;
  if (maxNear < lowest || maxNear > kPointMultiMaxNear) return fail(c, MOPTIX_ERR_INVALID, "maxNear out of range (1..64; 0 only with MOPTIX_POINT_MULTI_COUNT_ALL)");
  if (n > 0 && (!points || !counts || (maxNear > 0 && !hits))) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// As enqueue_points, with the same overflow area.  A launch takes at most kPointMaxLaunch / max(maxNear, 1) points, so that the index of
// a record within a launch fits 32 bits as the index of a point does.
int enqueue_points_multi(moptix_context c, const float* dPoints, int64_t n, int32_t maxNear, uint32_t flags, void* dHits, int32_t* dCounts) {
  PointMultiArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? pointkernel_overflow_entries(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->point.overflow.ensure(ovf), "alloc point query stack overflow area");
    a.stackOverflow = c->point.overflow.p;
  }
  a.maxNear = maxNear;
  const int64_t perLaunch = kPointMaxLaunch / (maxNear > 0 ? maxNear : 1);
  for (int64_t first = 0; first < n; first += perLaunch) {
    a.points = dPoints + 4 * first;
    a.hits = maxNear > 0 ? static_cast<char*>(dHits) + sizeof(moptix_point_hit) * (size_t)maxNear * (size_t)first : nullptr;
    a.counts = dCounts + first;
    a.n = (int)(n - first < perLaunch ? n - first : perLaunch);
    HIPCHK(c, launch_pointquery_multi(c->stream, a, nBlocks, (flags & MOPTIX_POINT_MULTI_COUNT_ALL) != 0), "launch K-nearest point query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_points_multi_device(moptix_context c, const float* dPoints, int64_t n, int32_t maxNear, uint32_t flags, void* dHits, int32_t* dCounts) {
  int rc = check_points_multi(c, dPoints, n, maxNear, flags, dHits, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dPoints) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dHits) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dCounts) & 3u) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "K-nearest point queries read points and write records 16 bytes at a time, counts 4: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_points_multi(c, dPoints, n, maxNear, flags, dHits, dCounts);
}

int moptix_query_points_multi(moptix_context c, const float* points, int64_t n, int32_t maxNear, uint32_t flags, moptix_point_hit* hits, int32_t* counts) {
  int rc = check_points_multi(c, points, n, maxNear, flags, hits, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t hitBytes = sizeof(moptix_point_hit) * (size_t)maxNear * (size_t)n, countBytes = sizeof(int32_t) * (size_t)n;      // counts behind the records
  HIPCHK(c, c->point.points.ensure(4 * (size_t)n), "alloc query points");
  HIPCHK(c, c->point.out.ensure(hitBytes + countBytes), "alloc point query results");
  HIPCHK(c, hipMemcpyAsync(c->point.points.p, points, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query points");
  int32_t* dCounts = reinterpret_cast<int32_t*>(c->point.out.p + hitBytes);
  if ((rc = enqueue_points_multi(c, c->point.points.p, n, maxNear, flags, c->point.out.p, dCounts)) != MOPTIX_OK) return rc;
  return read_back(c, { { maxNear > 0 ? hits : nullptr, c->point.out.p, hitBytes }, { counts, dCounts, countBytes } }, "read K-nearest point results");
}

int moptix_query_points_device(moptix_context c, const float* dPoints, int64_t n, int32_t mode, void* dOut) {
  int rc = check_points(c, dPoints, n, mode, dOut, true);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dPoints) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dOut) & (mode == MOPTIX_POINT_ANY ? 3u : 15u)) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "point queries read points and write records 16 bytes at a time: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_points(c, dPoints, n, mode, dOut);
}

static int query_points_host(moptix_context c, const float* points, int64_t n, int32_t mode, void* out, bool withSigned) {
  int rc = check_points(c, points, n, mode, out, withSigned);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t bytes = out_bytes(mode) * (size_t)n;
  HIPCHK(c, c->point.points.ensure(4 * (size_t)n), "alloc query points");
  HIPCHK(c, c->point.out.ensure(bytes), "alloc point query results");
  HIPCHK(c, hipMemcpyAsync(c->point.points.p, points, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query points");
  if ((rc = enqueue_points(c, c->point.points.p, n, mode, c->point.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->point.out.p, bytes } }, "read point query results");
}

int moptix_query_points(moptix_context c, const float* points, int64_t n, int32_t mode, void* out) {
  return query_points_host(c, points, n, mode, out, false);
}

int moptix_query_points_signed(moptix_context c, const float* points, int64_t n, moptix_point_hit* out) {
  return query_points_host(c, points, n, MOPTIX_POINT_SIGNED, out, true);
}

}  // extern "C"
