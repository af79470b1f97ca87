// api_radiance.hip -- radiance queries (radiancekernel.hip, pt_radiance.h): the two moptix_query_radiance* entry points of include/moptix.h.
#include <algorithm>
#include <cstring>

#include "api_context.h"
#include "pt_radiance.h"
#include "radiancekernel.h"

using namespace pt;
using namespace pt::api;

static_assert(MOPTIX_RADIANCE_CLAMP == RADIANCE_CLAMP, "radiance flags");

namespace {

int check_radiance(moptix_context c, const float* rays, int64_t n, const int32_t* seeds, const uint32_t* states, int32_t nSamples,
                   uint32_t flags, float* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0 || nSamples < 1) return fail(c, MOPTIX_ERR_INVALID, "bad ray or sample count");
  if ((flags & ~(uint32_t)MOPTIX_RADIANCE_CLAMP) != 0) return fail(c, MOPTIX_ERR_INVALID, "unknown radiance query flag");
  if (n > 0 && (!rays || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (n > 0 && (seeds != nullptr) == (states != nullptr))
    return fail(c, MOPTIX_ERR_INVALID, "a radiance query takes either a seed list or per-sample RNG states, not both and not neither");
  return MOPTIX_OK;
}

// The seeds' device copy.  The upload is asynchronous, so it reads a pinned staging of the context's; an event behind it says when the
// staging may be written again (a second query enqueued while the first has not started waits here for that one copy, for nothing else).
int upload_seeds(moptix_context c, const int32_t* seeds, int32_t nSamples) {
  moptix_context_t::Radiance& r = c->radiance;
  if (!r.seedsUploaded) HIPCHK(c, hipEventCreateWithFlags(&r.seedsUploaded, hipEventDisableTiming), "create event");
  else HIPCHK(c, hipEventSynchronize(r.seedsUploaded), "wait for the previous seed upload");
  if (r.seedStagingN < (size_t)nSamples) {
    if (r.seedStaging) (void)hipHostFree(r.seedStaging);
    r.seedStaging = nullptr; r.seedStagingN = 0;
    HIPCHK(c, hipHostMalloc((void**)&r.seedStaging, sizeof(int) * (size_t)nSamples, hipHostMallocDefault), "alloc seed staging");
    r.seedStagingN = (size_t)nSamples;
  }
  memcpy(r.seedStaging, seeds, sizeof(int) * (size_t)nSamples);
  HIPCHK(c, r.seeds.ensure((size_t)nSamples), "alloc radiance seeds");
  HIPCHK(c, hipMemcpyAsync(r.seeds.p, r.seedStaging, sizeof(int) * (size_t)nSamples, hipMemcpyHostToDevice, c->stream), "upload radiance seeds");
  HIPCHK(c, hipEventRecord(r.seedsUploaded, c->stream), "event");
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream.  The scratch holds `cap` per-sample records (option "radiance_buffer_mb"): a call with more
// samples runs in passes over the samples of all rays, or, where not even one sample of every ray fits, ray range after ray range with one
// sample per pass.  Every pass adds its samples in order onto the same output, so the cut changes no bit.
int enqueue_radiance(moptix_context c, const float* dRays, int64_t n, const int32_t* seeds, const uint32_t* dStates, int32_t nSamples,
                     uint32_t indexBase, uint32_t flags, float* dOut) {
  moptix_context_t::Radiance& r = c->radiance;
  RadianceArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  const size_t ovf = a.scene.rootRef != kEmptyRef ? radiancekernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, r.overflow.ensure(ovf), "alloc radiance stack overflow area");
    a.stackOverflow = r.overflow.p;
  }
  const long long cap = std::min<long long>((long long)c->opt.radianceBufferMB * (1ll << 16), kRadianceMaxWork);      // 16-byte records
  const long long perLaunch = std::min<long long>(n, cap);                                     // rays
  const int perPass = (int)std::max<long long>(1, std::min<long long>(nSamples, cap / perLaunch));      // samples
  HIPCHK(c, r.scratch.ensure(4 * (size_t)perLaunch * (size_t)perPass), "alloc radiance sample records");
  HIPCHK(c, r.work.ensure(1), "alloc radiance work counter");
  if (seeds) { const int rc = upload_seeds(c, seeds, nSamples); if (rc != MOPTIX_OK) return rc; }
  a.scratch = r.scratch.p; a.workCounter = r.work.p;
  a.statesStride = (size_t)nSamples; a.flags = flags;
  a.exitThreshold = c->opt.exitThreshold; a.leafThreshold = c->opt.leafThreshold;
  for (int64_t first = 0; first < n; first += perLaunch) {
    a.rays = dRays + 8 * first;
    a.out = dOut + 4 * first;
    a.n = (int)std::min<int64_t>(n - first, perLaunch);
    a.indexBase = indexBase + (uint32_t)(uint64_t)first;      // mod 2^32
    for (int s0 = 0; s0 < nSamples; s0 += perPass) {
      a.nSamples = std::min(perPass, nSamples - s0);
      a.seeds = seeds ? r.seeds.p + s0 : nullptr;
      a.states = dStates ? dStates + (size_t)first * (size_t)nSamples + (size_t)s0 : nullptr;
      a.firstPass = s0 == 0;
      HIPCHK(c, hipMemsetAsync(r.work.p, 0, sizeof(int), c->stream), "clear radiance work counter");
      HIPCHK(c, launch_radiance(c->stream, a, nBlocks), "launch radiance query");
    }
  }
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_query_radiance_device(moptix_context c, const float* dRays, int64_t n, const int32_t* seeds, const uint32_t* dStates,
                                 int32_t nSamples, uint32_t indexBase, uint32_t flags, float* dOut) {
  int rc = check_radiance(c, dRays, n, seeds, dStates, nSamples, flags, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dRays) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dOut) & 15u) != 0 || (reinterpret_cast<uintptr_t>(dStates) & 3u) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "radiance queries read rays and write results 16 bytes at a time: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_radiance(c, dRays, n, seeds, dStates, nSamples, indexBase, flags, dOut);
}

int moptix_query_radiance(moptix_context c, const float* rays, int64_t n, const int32_t* seeds, const uint32_t* states, int32_t nSamples,
                          uint32_t indexBase, uint32_t flags, float* out) {
  int rc = check_radiance(c, rays, n, seeds, states, nSamples, flags, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  moptix_context_t::Radiance& r = c->radiance;
  HIPCHK(c, r.rays.ensure(8 * (size_t)n), "alloc radiance rays");
  HIPCHK(c, r.out.ensure(4 * (size_t)n), "alloc radiance results");
  HIPCHK(c, hipMemcpyAsync(r.rays.p, rays, sizeof(float) * 8 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload radiance rays");
  if (states) {
    const size_t ns = (size_t)n * (size_t)nSamples;
    HIPCHK(c, r.states.ensure(ns), "alloc radiance states");
    HIPCHK(c, hipMemcpyAsync(r.states.p, states, sizeof(uint32_t) * ns, hipMemcpyHostToDevice, c->stream), "upload radiance states");
  }
  if ((rc = enqueue_radiance(c, r.rays.p, n, seeds, states ? r.states.p : nullptr, nSamples, indexBase, flags, r.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, r.out.p, sizeof(float) * 4 * (size_t)n } }, "read radiance results");
}

}  // extern "C"
