// api_segment.hip -- segment queries (segmentkernel.hip, pt_segment.h): the moptix_query_segments* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "segmentkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(moptix_segment_hit) == sizeof(SegmentHit), "moptix_segment_hit is the kernel's record");
static_assert(MOPTIX_SEGMENT_CLOSEST == SEGMENT_CLOSEST && MOPTIX_SEGMENT_ANY == SEGMENT_ANY, "segment query modes");

namespace {

size_t out_bytes(int32_t mode) { return mode == MOPTIX_SEGMENT_ANY ? sizeof(int32_t) : sizeof(moptix_segment_hit); }

int check_segments(moptix_context c, const float* segments, int64_t n, int32_t mode, const void* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_SEGMENT_CLOSEST && mode != MOPTIX_SEGMENT_ANY)) return fail(c, MOPTIX_ERR_INVALID, "bad segment count or query mode");
  if (n > 0 && (!segments || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kSegmentMaxLaunch segments.  The stack overflow area is the
// segment queries' own: allocated at the first segment query after a build, reused by every later one.
int enqueue_segments(moptix_context c, const float* dSegments, int64_t n, int32_t mode, void* dOut) {
  SegmentArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? segmentkernel_overflow_entries(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->segment.overflow.ensure(ovf), "alloc segment query stack overflow area");
    a.stackOverflow = c->segment.overflow.p;
  }
  for (int64_t first = 0; first < n; first += kSegmentMaxLaunch) {
    a.segments = dSegments + 8 * first;
    a.out = static_cast<char*>(dOut) + out_bytes(mode) * (size_t)first;
    a.n = (int)(n - first < kSegmentMaxLaunch ? n - first : kSegmentMaxLaunch);
    HIPCHK(c, launch_segmentquery(c->stream, a, nBlocks, mode), "launch segment query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_segments_device(moptix_context c, const float* dSegments, int64_t n, int32_t mode, void* dOut) {
  int rc = check_segments(c, dSegments, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dSegments) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dOut) & (mode == MOPTIX_SEGMENT_ANY ? 3u : 15u)) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "segment queries read segments and write records 16 bytes at a time: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_segments(c, dSegments, n, mode, dOut);
}

int moptix_query_segments(moptix_context c, const float* segments, int64_t n, int32_t mode, void* out) {
  int rc = check_segments(c, segments, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  const size_t bytes = out_bytes(mode) * (size_t)n;
  HIPCHK(c, c->segment.segments.ensure(8 * (size_t)n), "alloc query segments");
  HIPCHK(c, c->segment.out.ensure(bytes), "alloc segment query results");
  HIPCHK(c, hipMemcpyAsync(c->segment.segments.p, segments, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query segments");
  if ((rc = enqueue_segments(c, c->segment.segments.p, n, mode, c->segment.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->segment.out.p, bytes } }, "read segment query results");
}

}  // extern "C"
