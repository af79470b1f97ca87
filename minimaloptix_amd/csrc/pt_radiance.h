// pt_radiance.h -- radiance queries: the path-traced radiance that arrives along the caller's own rays (include/moptix.h "radiance queries").
//
// One sample is (ray i, sample s).  A ray is the ray queries' eight floats  ox oy oz dx dy dz tmin tmax  and is valid or not by the ray
// queries' rule (pt_query.h query_ray): a non-finite component, tmax <= tmin or a zero direction make it invalid, a negative tmin is walked
// as 0.  THE DIRECTION MUST BE UNIT LENGTH: it is used as given, the shading code (reflect, refract, the Disney terms, the light facing
// tests) and the sphere intersector assume |d| = 1, and nothing here or below renormalises it.
//
// A sample's path starts where begin_sample (pt_path.h) leaves a camera path -- depth 1, throughput (1, 1, 1), radiance (0, 0, 0), a
// radiance ray in flight -- with the caller's ray instead of the camera's and an RNG state that is either tea16(indexBase + i, seeds[s])
// (the camera's own rule, with the ray's index in the pixel's place) or handed over as it is.  The ray's own tmin and tmax hold for the
// first segment only: every later ray is what bounce / on_lights make.  From there the state machine is the render's, to the last
// bit: trace, on_result, on_lights, ... until end_sample; sc.maxDepth, sc.bg, the lights and sc.shadowNearest act as in a render.
//
// The sample's value is ps.rad as it stands (no clamp) or, with RADIANCE_CLAMP, ps.accum: Camera.cu:39's per-channel clamp to [0, 1].
// Its fourth component is the first segment's hit distance with the bits of the closest query's moptix_hit.t on the same ray: tbest of
// that segment, or the given tmax where it meets nothing or the ray is invalid.  An invalid ray's sample is (0, 0, 0, tmax) and no path
// is traced for it.
// Used by the radiance kernel (radiancekernel.hip) and by its CPU mirror (tests/hostsim/radiancesim.cpp); nothing of the render path includes it.
#pragma once
#include "pt_query.h"

namespace pt {

enum { RADIANCE_CLAMP = 1 };

// The RNG state of sample `seed` of ray `index` (indexBase + i, mod 2^32) in seeds mode: begin_sample's, the index in the pixel's place.
PT_HD uint32_t radiance_state(uint32_t index, int32_t seed) { return tea16(index, (uint32_t)seed); }

// r: the ray's eight floats, state: the path's RNG state.  A valid ray: the path stands in M_TRACE with its first segment in flight and
// ps.pixel = 1 marks that segment (radiance_on_result takes its distance).  An invalid ray: the sample is finished (M_NEW_SAMPLE) with
// value 0 and tFirst = the given tmax.
PT_HD void radiance_begin(const SceneView& sc, PathState& ps, const float r[8], uint32_t state, float& tFirst) {
  const bool valid = query_ray(r, ps);        // o, d, tmin (negative -> 0), tmax, kind = RK_RADIANCE
  ps.depth = 1; ps.seed = state;
  ps.thr = mk3(1.f, 1.f, 1.f); ps.rad = mk3(0.f, 0.f, 0.f); ps.accum = mk3(0.f, 0.f, 0.f);
  tFirst = ps.tmax;
  ps.pixel = valid ? 1 : 0;
  ps.mode = valid ? M_TRACE : M_NEW_SAMPLE;
}

// on_result for a path of a radiance query: the first segment's result also gives the sample's t (query_hit's rule).
template <bool CNT>
PT_HD void radiance_on_result(const SceneView& sc, PathState& ps, const Trav& tv, float& tFirst, Counters& ct) {
  if (ps.pixel != 0) { tFirst = tv.bestPrim < 0 ? ps.tmax : tv.tbest; ps.pixel = 0; }
  on_result<CNT>(sc, ps, tv, ct);
}

// The value of a finished sample (ps.mode == M_NEW_SAMPLE).
PT_HD v3 radiance_value(const PathState& ps, uint32_t flags) { return (flags & RADIANCE_CLAMP) ? ps.accum : ps.rad; }

// The ordered sum of a ray's samples: acc (+0 at the start of a ray, the output so far in a later pass) + v[0] + v[1] + ..., plain binary32
// adds in sample order.  v: the samples' records (r g b t), `stride` floats apart.
PT_HD v3 radiance_sum(v3 acc, const float* v, int nSamples, size_t stride) {
  for (int s = 0; s < nSamples; s++) {
    const float* p = v + (size_t)s * stride;
    acc = acc + mk3(p[0], p[1], p[2]);
  }
  return acc;
}

}  // namespace pt
