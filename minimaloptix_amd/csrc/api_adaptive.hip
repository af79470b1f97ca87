// api_adaptive.hip -- adaptive sampling (adaptivekernel.hip, pt_adaptive.h): the moptix_adaptive_* entry points and
// moptix_render_adaptive of include/moptix.h.  The per-pixel state lives in the context (api_context.h Adaptive); the passes go through
// the launch plan of api_render.hip (prepare_launch / launch_pass) with an order list and a reduction of their own, and through the
// trace kernels as they are: a pass whose order list starts with the active pixel slots and whose work count is nActive * nSeeds
// renders exactly those pixels (megakernel.h handout_to_item, "tile_major" 3).
#include <algorithm>
#include <cstring>

#include "adaptivekernel.h"
#include "api_context.h"

using namespace pt;
using namespace pt::api;

namespace {

void fill_args(moptix_context c, AdaptiveArgs& a) {
  moptix_context_t::Adaptive& s = c->ad;
  memset(&a, 0, sizeof(a));
  a.k.width = (int)c->params.width; a.k.height = (int)c->params.height;
  a.tilesX = (a.k.width + 7) / 8; a.nItems = a.tilesX * ((a.k.height + 7) / 8) * 64;
  a.accum = accum_ptr(c);
  a.count = s.count.p; a.moments = s.moments.p; a.error = s.error.p; a.converged = s.converged.p;
  a.key = s.order.keys.p; a.partials = reinterpret_cast<uint4*>(s.partials.p); a.totals = reinterpret_cast<AdaptiveTotals*>(s.totals.p);
}

// The state at this frame size: allocated and zeroed when there is none (first call, or dropped since).
int ensure_state(moptix_context c) {
  moptix_context_t::Adaptive& s = c->ad;
  const size_t px = (size_t)c->params.width * c->params.height;
  if (px > 0x7fffffffULL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  if (s.pixels == px) return MOPTIX_OK;
  HIPCHK(c, s.count.ensure(px), "alloc adaptive state");
  HIPCHK(c, s.moments.ensure(2 * px), "alloc adaptive state");
  HIPCHK(c, s.error.ensure(px), "alloc adaptive state");
  HIPCHK(c, s.converged.ensure(px), "alloc adaptive state");
  const size_t nGroups = (size_t)((c->params.width + 15) / 16) * ((c->params.height + 15) / 16);
  HIPCHK(c, s.partials.ensure(4 * nGroups), "alloc adaptive partials");
  HIPCHK(c, s.totals.ensure(4), "alloc adaptive totals");
  HIPCHK(c, hipMemsetAsync(s.count.p, 0, sizeof(uint32_t) * px, c->stream), "zero adaptive state");
  HIPCHK(c, hipMemsetAsync(s.moments.p, 0, sizeof(float) * 2 * px, c->stream), "zero adaptive state");
  HIPCHK(c, hipMemsetAsync(s.error.p, 0, sizeof(float) * px, c->stream), "zero adaptive state");
  HIPCHK(c, hipMemsetAsync(s.converged.p, 0, px, c->stream), "zero adaptive state");
  s.pixels = px; s.have = false;
  return MOPTIX_OK;
}

// Mask kernel (decide: pixels that need no more samples converge), then the order list: active slots first, deepest paths of earlier
// launches first, ties in slot order (the sort is stable).  Blocking: the host needs nActive for the next pass's work count.
int mask_and_order(moptix_context c, AdaptiveArgs& a, int decide, AdaptiveTotals& t) {
  moptix_context_t::Adaptive& s = c->ad;
  HIPCHK(c, launch_adaptive_mask(c->stream, a, decide), "launch adaptive mask");
  HIPCHK(c, s.order.sort(c->stream), "sort adaptive order");
  HIPCHK(c, hipMemcpyAsync(&t, s.totals.p, sizeof(t), hipMemcpyDeviceToHost, c->stream), "read adaptive totals");
  HIPCHK(c, hipStreamSynchronize(c->stream), "adaptive mask");
  return MOPTIX_OK;
}

hipError_t reduce_pass(hipStream_t stream, const LaunchArgs& la, void* user) {
  AdaptiveArgs a = *static_cast<const AdaptiveArgs*>(user);
  a.sampleBuf = la.sampleBuf; a.workCounter = la.workCounter; a.nSeeds = la.nSeeds;
  return launch_adaptive_reduce(stream, a);
}

// the entry points that read the state: it must exist at this frame size
int check_state(moptix_context c) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  if (c->ad.pixels == 0 || c->ad.pixels != (size_t)c->params.width * c->params.height)
    return fail(c, MOPTIX_ERR_STATE, "no adaptive state: moptix_render_adaptive or moptix_adaptive_clear first");
  return begin_call(c, true);
}

}  // namespace

extern "C" {

int moptix_adaptive_defaults(moptix_adaptive_params* out) {
  if (!out) return fail(nullptr, MOPTIX_ERR_INVALID, "null argument");
  out->threshold = 0.03f; out->minSamples = 16; out->batch = 64;
  return MOPTIX_OK;
}

int moptix_render_adaptive(moptix_context c, const int32_t* seeds, int32_t nSeeds, const moptix_adaptive_params* p, moptix_adaptive_stats* out) {
  if (out) memset(out, 0, sizeof(*out));
  if (!p) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (const char* why = ad_bad_params(p->threshold, p->minSamples, p->batch)) return fail(c, MOPTIX_ERR_INVALID, why);
  if (nSeeds < 0 || (nSeeds > 0 && !seeds)) return fail(c, MOPTIX_ERR_INVALID, "bad seeds");
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (c->rank != 0 || c->nRanks != 1)
    return fail(c, MOPTIX_ERR_STATE, "adaptive sampling renders the whole frame: a pixel's 3x3 window crosses into other ranks' tiles (moptix_set_partition(0, 1))");
  if (c->accumPlain) return fail(c, MOPTIX_ERR_STATE, "the accumulation buffer holds plain renders without per-pixel sample counts: moptix_adaptive_clear first");
  if ((rc = begin_call(c, true)) != MOPTIX_OK) return rc;
  if ((rc = ensure_state(c)) != MOPTIX_OK) return rc;
  moptix_context_t::Adaptive& s = c->ad;

  AdaptiveArgs a;
  fill_args(c, a);
  a.k.minSamples = p->minSamples; a.k.threshold = p->threshold;
  const uint64_t inFrame = (uint64_t)c->params.width * c->params.height;
  uint64_t passes = 0, traced = 0;
  AdaptiveTotals t = { 0u, 0u, 0u, 0u };
  if (nSeeds > 0) {
    RenderLaunch r;
    if ((rc = prepare_launch(c, nSeeds, false, true, r)) != MOPTIX_OK) return rc;
    if (r.p.nItems != a.nItems) return fail(c, MOPTIX_ERR_STATE, "launch plan and adaptive state disagree on the frame's pixel slots");
    HIPCHK(c, s.order.ensure(a.nItems, c->stream), "alloc adaptive order");      // the padding slots' keys stay at the 0 they are cleared to here
    a.key = s.order.keys.p;
    a.tileCost = r.a.tileCost;
    c->seedStaging.assign(seeds, seeds + nSeeds);
    HIPCHK(c, c->dSeeds.upload(c->seedStaging, c->stream), "upload seeds");
    // the active set as the state holds it (after a clear: every pixel), without deciding anything
    if ((rc = mask_and_order(c, a, 0, t)) != MOPTIX_OK) return rc;
    for (int first = 0; first < nSeeds && t.active > 0;) {
      const int n = ad_pass_seeds(s.have, p->minSamples, p->batch, nSeeds - first);
      for (long long sub = 0; sub < n; sub += r.perPass) {      // the per-sample buffer's budget cuts a pass, as it cuts moptix_render's
        const int m = (int)std::min<long long>(r.perPass, n - sub);
        PassOverride over = { s.order.order.p, (int)t.active * m, reduce_pass, &a };
        s.have = true;                                     // from here on the counts may describe samples in the accumulation buffer
        if ((rc = launch_pass(c, r, c->dSeeds.p + first + sub, m, &over)) != MOPTIX_OK) return rc;
        if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;
      }
      traced += (uint64_t)t.active * (uint64_t)n;
      first += n; passes++;
      if ((rc = mask_and_order(c, a, 1, t)) != MOPTIX_OK) return rc;
    }
  }
  if (nSeeds == 0) {      // nothing to render: the totals of the state as it is (no launch plan: the depth history is not read)
    HIPCHK(c, s.order.ensure(a.nItems, c->stream), "alloc adaptive order");      // the padding slots' keys stay at the 0 they are cleared to here
    a.key = s.order.keys.p;
    if ((rc = mask_and_order(c, a, 0, t)) != MOPTIX_OK) return rc;
  }
  if (out) {
    out->passes = passes; out->samplesTraced = traced; out->samplesUniform = inFrame * (uint64_t)nSeeds;
    out->activePixelsLast = t.active; out->convergedPixels = t.converged; out->minCount = t.minCount; out->maxCount = t.maxCount;
  }
  return MOPTIX_OK;
}

int moptix_adaptive_clear(moptix_context c) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  int rc = moptix_accum_clear(c);      // drops the state as well: ensure_state zeroes it
  if (rc != MOPTIX_OK) return rc;
  if ((rc = ensure_state(c)) != MOPTIX_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_adaptive_read(moptix_context c, const moptix_adaptive_buffers* d) {
  if (!c || !d) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_state(c);
  if (rc != MOPTIX_OK) return rc;
  const moptix_context_t::Adaptive& s = c->ad;
  return read_back(c, { { d->count, s.count.p, sizeof(uint32_t) * s.pixels }, { d->moments, s.moments.p, sizeof(float) * 2 * s.pixels },
                        { d->error, s.error.p, sizeof(float) * s.pixels }, { d->converged, s.converged.p, s.pixels } }, "read adaptive state");
}

int moptix_adaptive_mean_device(moptix_context c, float* dstDevice) {
  if (!c || !dstDevice) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_state(c);
  if (rc != MOPTIX_OK) return rc;
  AdaptiveArgs a;
  fill_args(c, a);
  HIPCHK(c, launch_adaptive_mean(c->stream, a, dstDevice), "launch adaptive mean");
  HIPCHK(c, hipStreamSynchronize(c->stream), "adaptive mean");
  return MOPTIX_OK;
}

int moptix_adaptive_mean(moptix_context c, float* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_state(c);
  if (rc != MOPTIX_OK) return rc;
  const size_t px = c->ad.pixels;
  HIPCHK(c, c->ad.mean.ensure(3 * px), "alloc adaptive mean");
  AdaptiveArgs a;
  fill_args(c, a);
  HIPCHK(c, launch_adaptive_mean(c->stream, a, c->ad.mean.p), "launch adaptive mean");
  return read_back(c, { { dstHost, c->ad.mean.p, sizeof(float) * 3 * px } }, "read adaptive mean");
}

int moptix_adaptive_resolve_rgb8(moptix_context c, uint8_t* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_state(c);
  if (rc != MOPTIX_OK) return rc;
  const size_t bytes = 3 * c->ad.pixels;
  HIPCHK(c, c->dRgb8.ensure(bytes), "alloc rgb8");
  AdaptiveArgs a;
  fill_args(c, a);
  HIPCHK(c, launch_adaptive_resolve_rgb8(c->stream, a, c->dRgb8.p), "adaptive resolve kernel");
  return read_back(c, { { dstHost, c->dRgb8.p, bytes } }, "read rgb8");
}

}  // extern "C"
