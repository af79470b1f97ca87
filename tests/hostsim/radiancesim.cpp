// radiancesim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the radiance-query kernel (minimaloptix_amd/csrc/radiancekernel.hip): the same
// per-sample code (pt_radiance.h over pt_path.h's state machine and traversal), compiled for the host and run one sample at a time, on the
// scene and tree of a hostsim_create handle (hostsim.h).  The GPU tests compare the kernel's output with this bit for bit.  It is not part
// of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_radiance.h"

using namespace hostsim;

namespace {

// One sample: its record r g b t.
template <bool N64>
void radiance_sample(const SceneView& sc, const float* r, uint32_t state, uint32_t flags, float rec[4]) {
  LocalStack st;
  Counters ct; memset(&ct, 0, sizeof(ct));
  PathState ps; memset(&ps, 0, sizeof(ps));
  Trav tv; memset(&tv, 0, sizeof(tv));
  float tFirst;
  radiance_begin(sc, ps, r, state, tFirst);
  while (ps.mode != M_NEW_SAMPLE) {
    if (ps.mode == M_TRACE) {
      trav_begin<false>(sc, ps, tv, ct);
      while (tv.node != kTravDone) trav_step<false, N64>(sc, ps, tv, st, ct);
      ps.mode = M_RESULT;
    } else if (ps.mode == M_RESULT) radiance_on_result<false>(sc, ps, tv, tFirst, ct);
    else on_lights<false>(sc, ps, ct);      // M_LIGHTS
  }
  const v3 v = radiance_value(ps, flags);
  rec[0] = v.x; rec[1] = v.y; rec[2] = v.z; rec[3] = tFirst;
}

}  // namespace

extern "C" {

// moptix_query_radiance on the CPU.  rays: n x 8 floats; seeds: nSamples launch seeds, or states: n x nSamples RNG states (exactly one
// of the two); out: n x 4 floats r g b t.
int radiancesim_query(void* h, int nodeFormat, const float* rays, int64_t n, const int32_t* seeds, const uint32_t* states, int32_t nSamples,
                      uint32_t indexBase, uint32_t flags, float* out) {
  if (!h || n < 0 || nSamples < 1 || (flags & ~(uint32_t)RADIANCE_CLAMP) != 0) return -1;
  if (n > 0 && (!rays || !out || (seeds != nullptr) == (states != nullptr))) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++) {
    const float* r = rays + 8 * (size_t)i;
    std::vector<float> rec(4 * (size_t)nSamples);
    for (int s = 0; s < nSamples; s++) {
      const uint32_t state = states ? states[(size_t)i * (size_t)nSamples + (size_t)s] : radiance_state(indexBase + (uint32_t)(uint64_t)i, seeds[s]);
      if (n64) radiance_sample<true>(sc, r, state, flags, &rec[4 * (size_t)s]);
      else radiance_sample<false>(sc, r, state, flags, &rec[4 * (size_t)s]);
    }
    const v3 acc = radiance_sum(mk3(0.f, 0.f, 0.f), rec.data(), nSamples, 4);
    float* o = out + 4 * (size_t)i;
    o[0] = acc.x; o[1] = acc.y; o[2] = acc.z; o[3] = rec[3];
  }
  return 0;
}

// Option "shadow_rule" on the handle: 0 = a shadow ray is blocked by an opaque Disney surface anywhere on its segment, whatever the scene
// holds; 1 (what hostsim_create sets up) = the nearest any-hit surface decides wherever the scene has a Disney GLASS material.
int radiancesim_shadow_rule(void* h, int rule) {
  if (!h || (rule != 0 && rule != 1)) return -1;
  HostScene& hs = static_cast<HostSim*>(h)->hs;
  hs.view.shadowNearest = 0;
  if (rule != 0)
    for (const DevMaterial& m : hs.mats) if (m.kind == MAT_DISNEY && m.brdfType == BRDF_GLASS) hs.view.shadowNearest = 1;
  return 0;
}

// For every pixel of the scene's frame: the ray begin_sample makes under `launchSeed` (rays[8 * pixel ..] = o, d, tmin, tmax) and the RNG
// state it leaves behind after the lens and jitter draws (states[pixel]) -- what a radiance query needs to walk the camera's own paths.
int radiancesim_camera(const hostsim_scene* s, int32_t launchSeed, float* rays, uint32_t* states) {
  if (!s || !rays || !states) return -1;
  SceneView sc; memset(&sc, 0, sizeof(sc));
  sc.width = (int)s->params.width; sc.height = (int)s->params.height;
  sc.epsT = s->params.rayEpsilonT; sc.cam = make_cam(s->params.cam);
  Counters ct; memset(&ct, 0, sizeof(ct));
  for (int pix = 0; pix < sc.width * sc.height; pix++) {
    PathState ps; memset(&ps, 0, sizeof(ps));
    ps.pixel = pix;
    begin_sample<false>(sc, ps, launchSeed, ct);
    float* r = rays + 8 * (size_t)pix;
    r[0] = ps.o.x; r[1] = ps.o.y; r[2] = ps.o.z; r[3] = ps.d.x; r[4] = ps.d.y; r[5] = ps.d.z; r[6] = ps.tmin; r[7] = ps.tmax;
    states[pix] = ps.seed;
  }
  return 0;
}

}  // extern "C"
