// api_aov.hip -- first-hit AOVs (aovkernel.hip, pt_aov.h): the buffers and the five moptix_*aov* entry points of include/moptix.h.
#include <cstring>

#include "aovkernel.h"
#include "api_context.h"

using namespace pt;
using namespace pt::api;

namespace pt { namespace api {
moptix_aov_buffers aov_ptrs(moptix_context c) {
  const moptix_aov_buffers& b = c->aov.bound;
  return moptix_aov_buffers{ b.albedo ? b.albedo : c->aov.albedo.p, b.normal ? b.normal : c->aov.normal.p, b.depth ? b.depth : c->aov.depth.p,
                             b.hits ? b.hits : c->aov.hits.p, b.primId ? b.primId : c->aov.primId.p, b.matId ? b.matId : c->aov.matId.p };
}
}}  // namespace pt::api

namespace {
int aov_zero(moptix_context c) {
  const size_t px = c->aov.pixels;
  const moptix_aov_buffers p = aov_ptrs(c);
  HIPCHK(c, hipMemsetAsync(p.albedo, 0, sizeof(float) * 3 * px, c->stream), "clear AOVs");
  HIPCHK(c, hipMemsetAsync(p.normal, 0, sizeof(float) * 3 * px, c->stream), "clear AOVs");
  HIPCHK(c, hipMemsetAsync(p.depth, 0, sizeof(float) * px, c->stream), "clear AOVs");
  HIPCHK(c, hipMemsetAsync(p.hits, 0, sizeof(float) * px, c->stream), "clear AOVs");
  HIPCHK(c, hipMemsetAsync(p.primId, 0xff, sizeof(int) * px, c->stream), "clear AOVs");      // -1
  HIPCHK(c, hipMemsetAsync(p.matId, 0xff, sizeof(int) * px, c->stream), "clear AOVs");
  c->aov.samples = 0;
  return MOPTIX_OK;
}
// The AOV buffers for the current frame size: allocated at the first AOV call (contexts that never ask for AOVs hold none), and
// cleared when the frame size changed since they were.
int ensure_aov(moptix_context c) {
  const size_t px = (size_t)c->params.width * c->params.height;
  const moptix_aov_buffers& b = c->aov.bound;
  if (!b.albedo) HIPCHK(c, c->aov.albedo.ensure(3 * px), "alloc AOVs");
  if (!b.normal) HIPCHK(c, c->aov.normal.ensure(3 * px), "alloc AOVs");
  if (!b.depth) HIPCHK(c, c->aov.depth.ensure(px), "alloc AOVs");
  if (!b.hits) HIPCHK(c, c->aov.hits.ensure(px), "alloc AOVs");
  if (!b.primId) HIPCHK(c, c->aov.primId.ensure(px), "alloc AOVs");
  if (!b.matId) HIPCHK(c, c->aov.matId.ensure(px), "alloc AOVs");
  if (c->aov.pixels == px) return MOPTIX_OK;
  c->aov.pixels = px;
  return aov_zero(c);
}
}  // namespace
extern "C" {

int moptix_render_aovs(moptix_context c, const int32_t* seeds, int32_t nSeeds) {
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (nSeeds < 0 || (nSeeds > 0 && !seeds)) return fail(c, MOPTIX_ERR_INVALID, "bad seeds");
  if ((rc = begin_call(c, false)) != MOPTIX_OK || (rc = ensure_aov(c)) != MOPTIX_OK) return rc;
  if (nSeeds == 0) { HIPCHK(c, hipStreamSynchronize(c->stream), "sync"); return MOPTIX_OK; }
  if ((long long)((c->params.width + 7) / 8) * ((c->params.height + 7) / 8) > 0x7fffffffLL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  AovArgs a;
  memset(&a, 0, sizeof(a));
  fill_view(c, a.scene);                                  // the whole frame: partition and node-format verdict are not consulted
  const bool node64 = c->bvh.nodes64 != nullptr && c->opt.nodeFormat != 128 && a.scene.rootRef != kEmptyRef;
  a.scene.nodes64 = node64 ? c->bvh.nodes64 : nullptr;
  std::vector<int> staged(seeds, seeds + nSeeds);
  HIPCHK(c, c->aov.seeds.upload(staged, c->stream), "upload AOV seeds");
  a.seeds = c->aov.seeds.p; a.nSeeds = nSeeds;
  a.writeIds = c->aov.samples == 0 ? 1 : 0;
  const moptix_aov_buffers p = aov_ptrs(c);
  a.albedo = p.albedo; a.normal = p.normal; a.depth = p.depth; a.hits = p.hits; a.primId = p.primId; a.matId = p.matId;
  const size_t ovf = aovkernel_overflow_ints(c->numCUs, c->bvh.stackBound);
  if (ovf > 0 && a.scene.rootRef != kEmptyRef) {
    HIPCHK(c, c->aov.overflow.ensure(ovf), "alloc AOV stack overflow area");
    a.stackOverflow = c->aov.overflow.p;
  }
  HIPCHK(c, c->aov.work.ensure(1), "alloc AOV tile counter");
  HIPCHK(c, launch_aovkernel(c->stream, a, c->numCUs, c->aov.work.p, node64), "launch AOV kernel");
  HIPCHK(c, hipStreamSynchronize(c->stream), "AOV kernel");     // also: `staged` dies here
  c->aov.samples += (uint64_t)nSeeds;
  return MOPTIX_OK;
}

int moptix_aov_clear(moptix_context c) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  int rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK || (rc = ensure_aov(c)) != MOPTIX_OK) return rc;
  if ((rc = aov_zero(c)) != MOPTIX_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_aov_samples(moptix_context c, uint64_t* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  *out = c->aov.samples;
  return MOPTIX_OK;
}

int moptix_aov_read(moptix_context c, const moptix_aov_buffers* dst) {
  if (!c || !dst) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  int rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK || (rc = ensure_aov(c)) != MOPTIX_OK) return rc;
  const size_t px = c->aov.pixels;
  const moptix_aov_buffers p = aov_ptrs(c);
  const size_t plane = sizeof(float) * px;      // the ids are 4 bytes a pixel as well
  return read_back(c, { { dst->albedo, p.albedo, 3 * plane }, { dst->normal, p.normal, 3 * plane }, { dst->depth, p.depth, plane },
                        { dst->hits, p.hits, plane }, { dst->primId, p.primId, plane }, { dst->matId, p.matId, plane } }, "read AOVs");
}

int moptix_aov_bind(moptix_context c, const moptix_aov_buffers* dstDevice) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  int rc;
  if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;
  c->aov.bound = dstDevice ? *dstDevice : moptix_aov_buffers{};
  c->aov.samples = 0;                 // the bound memory is taken as it is (moptix_aov_clear zeroes it)
  return MOPTIX_OK;
}

}  // extern "C"
