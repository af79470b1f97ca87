// api_box.hip -- box overlap queries (boxkernel.hip, pt_box.h): the moptix_query_boxes* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "boxkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(MOPTIX_BOX_ANY == BOX_ANY && MOPTIX_BOX_COUNT == BOX_COUNT, "box query modes");
static_assert(sizeof(long long) == sizeof(int64_t), "the kernel reads the offsets as long long");

namespace {

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_boxes(moptix_context c, const float* boxes, int64_t n, int32_t mode, const int32_t* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || (mode != MOPTIX_BOX_ANY && mode != MOPTIX_BOX_COUNT)) return fail(c, MOPTIX_ERR_INVALID, "bad box count or query mode");
  if (n > 0 && (!boxes || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

int check_boxes_list(moptix_context c, const float* boxes, int64_t n, const int64_t* offsets, const int32_t* prims, const int32_t* counts) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0) return fail(c, MOPTIX_ERR_INVALID, "bad box count");
  if (n > 0 && (!boxes || !offsets || !prims || !counts)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kBoxMaxLaunch boxes.  The stack overflow area is the box queries'
// own: allocated at the first box query after a build, reused by every later one.  mode BOX_LIST: dOut takes the counts.
int enqueue_boxes(moptix_context c, const float* dBoxes, int64_t n, int mode, int32_t* dOut, const int64_t* dOffsets, int32_t* dPrims) {
  BoxArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? boxkernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->box.overflow.ensure(ovf), "alloc box query stack overflow area");
    a.stackOverflow = c->box.overflow.p;
  }
  a.prims = dPrims;
  for (int64_t first = 0; first < n; first += kBoxMaxLaunch) {
    a.boxes = dBoxes + 6 * first;
    a.out = dOut + first;
    a.offsets = dOffsets ? reinterpret_cast<const long long*>(dOffsets) + first : nullptr;
    a.n = (int)(n - first < kBoxMaxLaunch ? n - first : kBoxMaxLaunch);
    HIPCHK(c, launch_boxquery(c->stream, a, nBlocks, mode), mode == BOX_LIST ? "launch box list query" : "launch box query");
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_boxes_device(moptix_context c, const float* dBoxes, int64_t n, int32_t mode, int32_t* dOut) {
  int rc = check_boxes(c, dBoxes, n, mode, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dBoxes, 7u) || misaligned(dOut, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "box queries read boxes 8 bytes at a time and write int32 results: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_boxes(c, dBoxes, n, mode, dOut, nullptr, nullptr);
}

int moptix_query_boxes(moptix_context c, const float* boxes, int64_t n, int32_t mode, int32_t* out) {
  int rc = check_boxes(c, boxes, n, mode, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  HIPCHK(c, c->box.boxes.ensure(6 * (size_t)n), "alloc query boxes");
  HIPCHK(c, c->box.out.ensure((size_t)n), "alloc box query results");
  HIPCHK(c, hipMemcpyAsync(c->box.boxes.p, boxes, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query boxes");
  if ((rc = enqueue_boxes(c, c->box.boxes.p, n, mode, c->box.out.p, nullptr, nullptr)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->box.out.p, sizeof(int32_t) * (size_t)n } }, "read box query results");
}

int moptix_query_boxes_list_device(moptix_context c, const float* dBoxes, int64_t n, const int64_t* dOffsets, int32_t* dPrims, int32_t* dCounts) {
  int rc = check_boxes_list(c, dBoxes, n, dOffsets, dPrims, dCounts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dBoxes, 7u) || misaligned(dOffsets, 7u) || misaligned(dPrims, 3u) || misaligned(dCounts, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "box list queries read boxes and offsets 8 bytes at a time and write int32 ids and counts: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_boxes(c, dBoxes, n, BOX_LIST, dCounts, dOffsets, dPrims);
}

int moptix_query_boxes_list(moptix_context c, const float* boxes, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts) {
  int rc = check_boxes_list(c, boxes, n, offsets, prims, counts);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (offsets[0] < 0) return fail(c, MOPTIX_ERR_INVALID, "offsets[0] must be >= 0");
  for (int64_t i = 0; i < n; i++)
    if (offsets[i + 1] < offsets[i]) return fail(c, MOPTIX_ERR_INVALID, "offsets must not decrease");
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  // the staging of prims covers 0 .. offsets[n], so that the caller's offsets serve as they are; the slices' span is read back
  const size_t lo = (size_t)offsets[0], hi = (size_t)offsets[n];
  HIPCHK(c, c->box.boxes.ensure(6 * (size_t)n), "alloc query boxes");
  HIPCHK(c, c->box.offsets.ensure((size_t)n + 1), "alloc box list offsets");
  HIPCHK(c, c->box.prims.ensure(hi), "alloc box list ids");
  HIPCHK(c, c->box.out.ensure((size_t)n), "alloc box query results");
  HIPCHK(c, hipMemcpyAsync(c->box.boxes.p, boxes, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query boxes");
  HIPCHK(c, hipMemcpyAsync(c->box.offsets.p, offsets, sizeof(int64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream), "upload box list offsets");
  if ((rc = enqueue_boxes(c, c->box.boxes.p, n, BOX_LIST, c->box.out.p, reinterpret_cast<const int64_t*>(c->box.offsets.p), c->box.prims.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { hi > lo ? prims + lo : nullptr, c->box.prims.p + lo, sizeof(int32_t) * (hi - lo) }, { counts, c->box.out.p, sizeof(int32_t) * (size_t)n } },
                   "read box list results");
}

}  // extern "C"
