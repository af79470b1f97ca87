// api_denoise.hip -- the denoiser (denoisekernel.hip, pt_denoise.h): the four moptix_denoise* entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "denoisekernel.h"

using namespace pt;
using namespace pt::api;

extern "C" {

int moptix_denoise_defaults(moptix_denoise_params* out) {
  if (!out) return fail(nullptr, MOPTIX_ERR_INVALID, "null argument");
  out->iterations = 5; out->normalPower = 128; out->demodulate = 0;
  out->sigmaLuminance = 4.0f; out->sigmaDepth = 1.0f;
  return MOPTIX_OK;
}

int moptix_denoise(moptix_context c, const moptix_denoise_params* p, float nAccumulation) {
  if (!c || !p) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!(nAccumulation > 0.0f) || !__builtin_isfinite(nAccumulation)) return fail(c, MOPTIX_ERR_INVALID, "nAccumulation must be > 0");
  if (p->iterations < 0 || p->iterations > 8) return fail(c, MOPTIX_ERR_INVALID, "iterations in [0,8]");
  if (p->normalPower < 1 || p->normalPower > 256) return fail(c, MOPTIX_ERR_INVALID, "normalPower in [1,256]");
  if (p->demodulate != 0 && p->demodulate != 1) return fail(c, MOPTIX_ERR_INVALID, "demodulate is 0 or 1");
  if (!(p->sigmaLuminance >= 0.0f) || !__builtin_isfinite(p->sigmaLuminance) || !(p->sigmaDepth >= 0.0f) || !__builtin_isfinite(p->sigmaDepth))
    return fail(c, MOPTIX_ERR_INVALID, "sigmas must be finite and >= 0");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "moptix_set_params has not been called");
  if (c->aov.samples == 0) return fail(c, MOPTIX_ERR_STATE, "no AOV samples: moptix_render_aovs first");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;       // a beauty batch still in flight finishes (and is timed) first
  if ((rc = ensure_accum(c)) != MOPTIX_OK) return rc;
  const size_t px = (size_t)c->params.width * c->params.height;
  if (px > 0x7fffffffULL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  HIPCHK(c, c->dn.colA.ensure(px), "alloc denoiser");
  HIPCHK(c, c->dn.colB.ensure(px), "alloc denoiser");
  HIPCHK(c, c->dn.guide.ensure(px), "alloc denoiser");
  HIPCHK(c, c->dn.side.ensure(px), "alloc denoiser");
  if (!c->dn.bound) HIPCHK(c, c->dn.out.ensure(3 * px), "alloc denoiser output");
  DenoiseArgs a;
  memset(&a, 0, sizeof(a));
  a.k.width = (int)c->params.width; a.k.height = (int)c->params.height; a.k.normalPower = p->normalPower;
  a.k.sigmaLuminance = p->sigmaLuminance; a.k.sigmaDepth = p->sigmaDepth;
  const moptix_aov_buffers b = aov_ptrs(c);
  a.accum = accum_ptr(c); a.albedo = b.albedo; a.normal = b.normal; a.depth = b.depth; a.hits = b.hits;
  a.nAccumulation = nAccumulation; a.nSamples = (float)c->aov.samples;
  a.iterations = p->iterations; a.demodulate = p->iterations > 0 ? p->demodulate : 0;
  a.colA = c->dn.colA.p; a.colB = c->dn.colB.p; a.guide = c->dn.guide.p; a.side = c->dn.side.p;
  a.out = c->dn.bound ? c->dn.bound : c->dn.out.p;
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
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  int rc;
  if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;
  const float* src = c->dn.bound ? c->dn.bound : c->dn.out.p;
  if (!src) return fail(c, MOPTIX_ERR_STATE, "the own output buffer holds nothing (it was bound when the denoiser last ran)");
  HIPCHK(c, hipMemcpyAsync(dstHost, src, sizeof(float) * 3 * px, hipMemcpyDeviceToHost, c->stream), "read denoiser output");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_denoise_bind(moptix_context c, float* dstDevice) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  int rc;
  if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc;
  c->dn.bound = dstDevice;
  return MOPTIX_OK;
}

}  // extern "C"
