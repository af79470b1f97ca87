// api_denoise.hip -- the denoiser (denoisekernel.hip, pt_denoise.h): the four moptix_denoise* entry points of include/moptix.h, and
// what moptix_denoise_temporal (api_temporal.hip) shares with moptix_denoise: context checks, scratch, constants, output.
#include <cstring>

#include "api_context.h"
#include "denoisekernel.h"

using namespace pt;
using namespace pt::api;

namespace pt { namespace api {

int denoise_begin(moptix_context c, bool ownGuide, size_t& px) {
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "moptix_set_params has not been called");
  if (c->aov.samples == 0) return fail(c, MOPTIX_ERR_STATE, "no AOV samples: moptix_render_aovs first");
  const int rc = begin_call(c, true);      // a beauty batch still in flight finishes (and is timed) first
  if (rc != MOPTIX_OK) return rc;
  px = (size_t)c->params.width * c->params.height;
  if (px > 0x7fffffffULL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  HIPCHK(c, c->dn.colA.ensure(px), "alloc denoiser");
  HIPCHK(c, c->dn.colB.ensure(px), "alloc denoiser");
  if (ownGuide) HIPCHK(c, c->dn.guide.ensure(px), "alloc denoiser");
  HIPCHK(c, c->dn.side.ensure(px), "alloc denoiser");
  if (!c->dn.bound) HIPCHK(c, c->dn.out.ensure(3 * px), "alloc denoiser output");
  return MOPTIX_OK;
}

void denoise_consts(moptix_context c, const moptix_denoise_params* p, DenoiseConsts& k) {
  k.width = (int)c->params.width; k.height = (int)c->params.height; k.normalPower = p->normalPower;
  k.sigmaLuminance = p->sigmaLuminance; k.sigmaDepth = p->sigmaDepth;
}

}}  // namespace pt::api

extern "C" {

int moptix_denoise_defaults(moptix_denoise_params* out) {
  if (!out) return fail(nullptr, MOPTIX_ERR_INVALID, "null argument");
  out->iterations = 5; out->normalPower = 128; out->demodulate = 0;
  out->sigmaLuminance = 4.0f; out->sigmaDepth = 1.0f;
  return MOPTIX_OK;
}

int moptix_denoise(moptix_context c, const moptix_denoise_params* p, float nAccumulation) {
  if (!c || !p) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (const char* why = dn_bad_params(nAccumulation, p->iterations, p->normalPower, p->demodulate, p->sigmaLuminance, p->sigmaDepth))
    return fail(c, MOPTIX_ERR_INVALID, why);
  size_t px;
  const int rc = denoise_begin(c, true, px);
  if (rc != MOPTIX_OK) return rc;
  DenoiseArgs a;
  memset(&a, 0, sizeof(a));
  denoise_consts(c, p, a.k);
  const moptix_aov_buffers b = aov_ptrs(c);
  a.accum = accum_ptr(c); a.albedo = b.albedo; a.normal = b.normal; a.depth = b.depth; a.hits = b.hits;
  a.nAccumulation = nAccumulation; a.nSamples = (float)c->aov.samples;
  a.iterations = p->iterations; a.demodulate = p->iterations > 0 ? p->demodulate : 0;
  a.colA = c->dn.colA.p; a.colB = c->dn.colB.p; a.guide = c->dn.guide.p; a.side = c->dn.side.p;
  a.out = denoise_out(c);
  HIPCHK(c, launch_denoise(c->stream, a), "launch denoiser");
  HIPCHK(c, hipStreamSynchronize(c->stream), "denoiser");
  c->dn.pixels = px;
  return MOPTIX_OK;
}

int moptix_denoise_read(moptix_context c, float* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  const size_t px = (size_t)c->params.width * c->params.height;
  if (c->dn.pixels != px) return fail(c, MOPTIX_ERR_STATE, "nothing denoised at this frame size");
  const int rc = begin_call(c, false);
  if (rc != MOPTIX_OK) return rc;
  if (!denoise_out(c)) return fail(c, MOPTIX_ERR_STATE, "the own output buffer holds nothing (it was bound when the denoiser last ran)");
  return read_back(c, { { dstHost, denoise_out(c), sizeof(float) * 3 * px } }, "read denoiser output");
}

int moptix_denoise_bind(moptix_context c, float* dstDevice) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  int rc;
  if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;
  c->dn.bound = dstDevice;
  return MOPTIX_OK;
}

}  // extern "C"
