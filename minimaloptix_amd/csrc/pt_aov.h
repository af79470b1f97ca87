// pt_aov.h -- first-hit AOVs (albedo, normal, depth, ids) of the primary rays the beauty pass traces.
//
// For a (pixel, launch seed) the camera ray is begin_sample's, bit for bit (same lens and jitter draws of the RNG), its closest hit
// is found with the traversal of pt_path.h (rule D5: nearest t, then the lower primitive id), and one sample of every AOV is taken
// from that hit:
//   albedo  the colour of the hit's program: Lambertian / metal / glass -> albedo; Disney non-glass -> Cdlin (srgb2lin of the texel
//           when textured, as on_lights uses it); Disney glass -> the tint glass_body multiplies by (colour or raw texel);
//           light -> clamp(emission, 0, 1); miss -> the background colour
//   normal  faceforward(shadingNormal, -d, geoNormal): world space, facing the camera; miss -> (0,0,0)
//   depth   t of the hit along the normalised direction from the lens point; miss -> nothing
//   hits    1 per hit; miss -> nothing
//   ids     primitive id (spheres, quads, triangles in upload order) and material id of the hit, -1 on a miss
// The per-pixel sums are added in seed order, so calls with seed lists A and B give the bits of one call with A + B.
// Used by the AOV kernel (aovkernel.hip) and by its CPU mirror (tests/aovsim); nothing of the beauty pass includes it.
#pragma once
#include "pt_path.h"

namespace pt {

// one sample's contribution
struct AovSample { v3 albedo, normal; float t; int prim, mat; bool hit; };

// The hit the traversal left in tv (tv.bestPrim < 0: a miss) -> the sample's AOVs.  Reads what on_result reads, in the same way.
PT_HD void aov_sample(const SceneView& sc, const PathState& ps, const Trav& tv, AovSample& s) {
  if (tv.bestPrim < 0) {                                           // staticMiss, miss.cu:10-12
    s.albedo = sc.bg; s.normal = mk3(0.f, 0.f, 0.f); s.t = 0.f; s.prim = -1; s.mat = -1; s.hit = false;
    return;
  }
  HitAttr h;
  hit_attributes(sc, ps, tv, h);
  const DevMaterial m = load_const(at32(sc.mats, h.mat));
  v3 albedo;
  if (m.kind == MAT_LIGHT) albedo = mk3(clampf(m.emission.x, 0.f, 1.f), clampf(m.emission.y, 0.f, 1.f), clampf(m.emission.z, 0.f, 1.f));
  else if (m.kind != MAT_DISNEY) albedo = m.albedo;                // lambertian, metal, glass: the throughput factor of the bounce
  else {                                                           // disney, Material.cu:128-132
    const bool textured = m.albedoTex != 0;
    const v3 baseColor = textured ? xyz(tex2d(sc.textures[m.albedoTex - 1], h.texu, h.texv)) : m.color;
    if (m.brdfType == BRDF_GLASS) albedo = baseColor;             // glass_body's tint
    else albedo = textured ? srgb2lin(baseColor) : m.Cdlin;        // on_lights' Cdlin
  }
  s.albedo = albedo;
  s.normal = faceforward(h.shadingNormal, -ps.d, h.geoNormal);
  s.t = tv.tbest; s.prim = tv.bestPrim; s.mat = h.mat; s.hit = true;
}

// A pixel's running sums.  writeIds: this is the first sample after a clear -- the ids are taken from it.
struct AovPixel { v3 albedo, normal; float depth, hits; int prim, mat; };
PT_HD void aov_add(AovPixel& p, const AovSample& s, bool writeIds) {
  p.albedo = p.albedo + s.albedo;
  p.normal = p.normal + s.normal;
  if (s.hit) { p.depth = p.depth + s.t; p.hits = p.hits + 1.0f; }
  if (writeIds) { p.prim = s.prim; p.mat = s.mat; }
}

}  // namespace pt
