/*
 * pt_oracle.c -- CPU ORACLE (test infrastructure only; see pt_oracle.h header).
 *
 * Structure deliberately follows the reference: a *recursive* closest-hit
 * evaluation, one function per OptiX program, brute-force lists for analytic
 * primitives and an independent median-split BVH for triangles.  The HIP
 * product path is organised completely differently (iterative, LBVH, LDS
 * stack); agreement between the two is the parity evidence.
 *
 * Every function cites the reference file:line it restates
 * (paths relative to /root/reference/MinimalOptiX/).
 */
#include "pt_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------ math -- */
typedef struct { float x, y, z; } f3;

static inline f3 mk3(float x, float y, float z) { f3 r = { x, y, z }; return r; }
static inline f3 ld3(const float* p) { return mk3(p[0], p[1], p[2]); }
static inline void st3(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
static inline f3 add3(f3 a, f3 b) { return mk3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline f3 sub3(f3 a, f3 b) { return mk3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline f3 mul3(f3 a, f3 b) { return mk3(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline f3 scl3(f3 a, float s) { return mk3(a.x * s, a.y * s, a.z * s); }
static inline f3 neg3(f3 a) { return mk3(-a.x, -a.y, -a.z); }
static inline f3 adds3(f3 a, float s) { return mk3(a.x + s, a.y + s, a.z + s); }
/* AC3: optix float3/float multiplies by the reciprocal */
static inline f3 divs3(f3 a, float s) { float inv = 1.0f / s; return scl3(a, inv); }
/* AC1 */
static inline float dot3(f3 a, f3 b) { return fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)); }
/* AC2 */
static inline f3 cross3(f3 a, f3 b) {
  return mk3(fmaf(a.y, b.z, -(a.z * b.y)), fmaf(a.z, b.x, -(a.x * b.z)), fmaf(a.x, b.y, -(a.y * b.x)));
}
static inline float len3(f3 a) { return sqrtf(dot3(a, a)); }
static inline f3 norm3(f3 a) { float inv = 1.0f / sqrtf(dot3(a, a)); return scl3(a, inv); }
/* AC7 */
static inline f3 ray_at(f3 o, f3 d, float t) { return mk3(fmaf(t, d.x, o.x), fmaf(t, d.y, o.y), fmaf(t, d.z, o.z)); }
static inline float lerpf(float a, float b, float t) { return a + t * (b - a); }          /* A1 lerp */
static inline f3 lerp3(f3 a, f3 b, float t) { return add3(a, scl3(sub3(b, a), t)); }
static inline float clampf(float x, float lo, float hi) { return fmaxf(lo, fminf(x, hi)); }
static inline float sqr(float x) { return x * x; }                                          /* utils_device.h:145 */
/* AC5: sin and cos by the contract's binary32 algorithm (quadrant, 3-step Cody-Waite reduction with fma,
 * degree-7/8 kernels on |r| <= pi/4, quadrant fix-up); written out here independently of the kernels */
static inline void sincos_ac(float x, float* s, float* c) {
  const float qf = floorf(fmaf(x, 0.636619772f, 0.5f));
  float r = fmaf(qf, -1.5703125f, x);
  r = fmaf(qf, -4.837512969970703125e-4f, r);
  r = fmaf(qf, -7.54978995489188216e-8f, r);
  const float z = r * r;
  const float sp = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
  const float cp = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
  const float sr = fmaf(sp * z, r, r);
  const float cr = fmaf(cp * z, z, fmaf(-0.5f, z, 1.0f));
  switch ((int)qf & 3) {
    case 0: *s = sr; *c = cr; break;
    case 1: *s = cr; *c = -sr; break;
    case 2: *s = -sr; *c = -cr; break;
    default: *s = -cr; *c = sr; break;
  }
}
void orc_sincos(float x, float* s, float* c) { sincos_ac(x, s, c); }
void orc_sincos_n(const float* x, float* s, float* c, long n) { for (long i = 0; i < n; i++) sincos_ac(x[i], &s[i], &c[i]); }

#define ORC_PI 3.14159265358979323846f  /* M_PIf */
#define ORC_RT_DEFAULT_MAX 1e27f

/* A1: reflect / faceforward / refract */
static inline f3 reflect3(f3 i, f3 n) { return sub3(i, scl3(scl3(n, 2.0f), dot3(n, i))); }
static inline f3 faceforward3(f3 n, f3 i, f3 nref) { return scl3(n, copysignf(1.0f, dot3(i, nref))); }
static int refract3(f3* r, f3 i, f3 n, float ior) {
  f3 nn = n;
  float negNdotV = dot3(i, nn);
  float eta;
  if (negNdotV > 0.0f) { eta = ior; nn = neg3(n); negNdotV = -negNdotV; }
  else { eta = 1.0f / ior; }
  const float k = 1.0f - eta * eta * (1.0f - negNdotV * negNdotV);
  if (k < 0.0f) { *r = mk3(0.f, 0.f, 0.f); return 0; }
  *r = norm3(sub3(scl3(i, eta), scl3(nn, eta * negNdotV + sqrtf(k))));
  return 1;
}

/* A1: Onb */
typedef struct { f3 tangent, binormal, normal; } Onb;
static Onb onb_make(f3 n) {
  Onb o; o.normal = n;
  if (fabsf(n.x) > fabsf(n.z)) o.binormal = mk3(-n.y, n.x, 0.f);
  else                         o.binormal = mk3(0.f, -n.z, n.y);
  o.binormal = norm3(o.binormal);
  o.tangent = cross3(o.binormal, o.normal);
  return o;
}
static inline f3 onb_inverse(const Onb* o, f3 p) {
  return add3(add3(scl3(o->tangent, p.x), scl3(o->binormal, p.y)), scl3(o->normal, p.z));
}

/* ------------------------------------------------------------------- RNG -- */
/* utils_device.h:8-22 tea<16> */
uint32_t orc_tea16(uint32_t val0, uint32_t val1) {
  uint32_t v0 = val0, v1 = val1, s0 = 0;
  for (unsigned n = 0; n < 16; n++) {
    s0 += 0x9e3779b9u;
    v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
    v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
  }
  return v0;
}
/* utils_device.h:24-29 */
uint32_t orc_lcg(int32_t* seed) {
  uint32_t s = (uint32_t)*seed;
  s = 1664525u * s + 1013904223u;
  *seed = (int32_t)s;
  return s & 0x00FFFFFFu;
}
/* utils_device.h:32-34 */
float orc_rand(int32_t* seed) { return (float)orc_lcg(seed) / (float)0x01000000; }
/* launchSeed(i) = (int)tea<16>(i, baseSeed) */
int32_t orc_launch_seed(uint32_t i, uint32_t baseSeed) { return (int32_t)orc_tea16(i, baseSeed); }

/* utils_device.h:36-43 */
static int g_disney_binary64 = 0;
/* ANALYSIS switches for the comparison with demo/coffee.png (DESIGN.md "coffee.png pin"); all off = the restated reference.
 *   indirect_scale_pct : the BRDF-bounce term of the disney program (Material.cu:217-219) is multiplied by pct/100 at every depth
 *   indirect_depth1_off: ... is dropped at the camera-visible hit only (what is left is emission + next-event estimation there)
 *   shadow_leak_pct    : a shadow ray that an opaque surface would block gets through with this probability (in 1/100 %) */
static int g_indirect_scale_pct = 100, g_indirect_depth1_off = 0;
/*   draw_order         : C++ leaves the evaluation order of `a * rand(s) + b * rand(s)` and of function arguments unspecified
 *                        (SURVEY A2 assumes left to right).  bit 0: the quad light's two draws swapped (Material.cu:180),
 *                        bit 1: cosine_sample_hemisphere's two arguments swapped (disney.h:13), bit 2: the camera's jitter pair (Camera.cu:28) */
static int g_draw_order = 0;
/*   noshadow_first/last: materials with an index in [first, last] do not stop shadow rays (which occluder class casts the
 *                        shadows that differ from the PNG?) */
static int g_noshadow_first = 1, g_noshadow_last = 0;
/*   shadow_any_opaque_blocks : rounds 1-2 defined a shadow ray by SURVEY A2's order-independent rule (an opaque Disney surface
 *                         ANYWHERE on the segment zeroes it, every glass surface crossed multiplies by its colour).  Since round 3
 *                         the default is what OptiX does with a front-to-back traversal (see shadow_attenuation); this switch
 *                         brings the old rule back for comparison. */
static int g_shadow_any_opaque_blocks = 0;
/*   cos_short_tenth_ulp : disneyPdf's cosTheta = |N.H| is multiplied by (1 - k/10 * 2^-24).  The reference is built with
 *                         -use_fast_math: normalize() is v * (1 / sqrt(.)) with rsqrt / division approximations of a few ulp, so N and H
 *                         are not unit vectors to better than ~1e-7 -- and GTR2's 1 + (a^2 - 1) cos^2 with a^2 = 1e-6 (Plastic_Orange)
 *                         turns a shortfall of ONE ulp of the cosine into +12 % of t at the lobe's peak.  Models a systematic shortfall. */
static int g_cos_short_tenth_ulp = 0;

static f3 rand_in_unit_sphere(int32_t* seed) {
  f3 res;
  do {
    float a = orc_rand(seed), b = orc_rand(seed), c = orc_rand(seed);
    res = sub3(scl3(mk3(a, b, c), 2.0f), mk3(1.f, 1.f, 1.f));
  } while (len3(res) >= 1.0f);
  return res;
}
/* utils_device.h:45-52 */
static f3 rand_in_unit_disk(int32_t* seed) {
  f3 res;
  do {
    float a = orc_rand(seed), b = orc_rand(seed);
    res = sub3(scl3(mk3(a, b, 0.f), 2.0f), mk3(1.f, 1.f, 0.f));
  } while (len3(res) >= 1.0f);
  return res;
}

/* --------------------------------------------------------- host helpers -- */
/* utils_host.cpp:77-99 */
void orc_set_cam_params(const float from[3], const float at[3], const float upv[3],
                        float vFoV, float aspect, float aperture, float focus, OrcCam* cam) {
  static const float pi = 3.141592653589793238462643383279502884f;
  f3 lookFrom = ld3(from), lookAt = ld3(at), up = ld3(upv);
  float theta = vFoV * pi / 180;
  float halfHeight = tanf(theta / 2);   /* `tan(float)` resolves to the float overload in C++ */
  float halfWidth = aspect * halfHeight;
  f3 w = norm3(sub3(lookFrom, lookAt));
  f3 u = norm3(cross3(up, w));
  f3 v = cross3(w, u);
  f3 ll = sub3(sub3(sub3(lookFrom, scl3(u, focus * halfWidth)), scl3(v, focus * halfHeight)), scl3(w, focus));
  f3 horizontal = scl3(u, 2 * focus * halfWidth);
  f3 vertical = scl3(v, 2 * focus * halfHeight);
  st3(cam->origin, lookFrom); st3(cam->horizontal, horizontal); st3(cam->vertical, vertical);
  st3(cam->scrLowerLeftCorner, ll); st3(cam->u, u); st3(cam->v, v);
  cam->lensRadius = aperture / 2;
}
/* utils_host.cpp:67-75 */
void orc_set_quad_params(const float anchor[3], const float v1a[3], const float v2a[3], OrcQuad* q) {
  f3 a = ld3(anchor), v1 = ld3(v1a), v2 = ld3(v2a);
  f3 normal = norm3(cross3(v2, v1));
  float d = dot3(normal, a);
  q->plane[0] = normal.x; q->plane[1] = normal.y; q->plane[2] = normal.z; q->plane[3] = d;
  st3(q->v1, divs3(v1, dot3(v1, v1)));
  st3(q->v2, divs3(v2, dot3(v2, v2)));
  st3(q->anchor, a);
}
/* utils_host.cpp:101-116 */
void orc_init_disney(OrcMaterial* m) {
  memset(m, 0, sizeof(*m));
  m->kind = ORC_DISNEY;
  m->color[0] = m->color[1] = m->color[2] = 1.0f;
  m->metallic = 0.0f; m->subsurface = 0.0f; m->specular = 0.5f; m->roughness = 0.5f;
  m->specularTint = 0.0f; m->anisotropic = 0.0f; m->sheen = 0.0f; m->sheenTint = 0.5f;
  m->clearcoat = 0.0f; m->clearcoatGloss = 1.0f; m->brdfType = ORC_BRDF_NORMAL; m->albedoID = 0;
}

/* -------------------------------------------------- utils_device helpers -- */
/* utils_device.h:63-67 */
static float fresnel(float cosThetaI, float cosThetaT, float refIdx) {
  float rs = (cosThetaI - cosThetaT * refIdx) / (cosThetaI + refIdx * cosThetaT);
  float rp = (cosThetaI * refIdx - cosThetaT) / (cosThetaI * refIdx + cosThetaT);
  return 0.5f * (rs * rs + rp * rp);
}
static inline int32_t f2i(float f) { int32_t i; memcpy(&i, &f, 4); return i; }
static inline float i2f(int32_t i) { float f; memcpy(&f, &i, 4); return f; }
/* utils_device.h:82-104 */
static float offset1(float h, float n) {
  const float epsilon = 1.0e-4f;
  const float offs = 4096.0f * 2.0f;
  if ((f2i(h) & 0x7fffffff) < f2i(epsilon)) return h + epsilon * n;
  return i2f(f2i(h) + (int32_t)(copysignf(offs, h) * n));
}
static f3 offset_pt(f3 p, f3 n) { return mk3(offset1(p.x, n.x), offset1(p.y, n.y), offset1(p.z, n.z)); }
void orc_offset(const float p[3], const float n[3], float out[3]) { st3(out, offset_pt(ld3(p), ld3(n))); }
/* utils_device.h:72-79 */
static float intersect_plane(f3 origin, f3 direction, f3 normal, f3 point) {
  return -(dot3(normal, sub3(origin, point))) / dot3(normal, direction);
}
/* utils_device.h:108-128 */
static void refine_hitpoint(f3 original, f3 direction, f3 normal, f3 p, f3* back, f3* front) {
  float refined_t = intersect_plane(original, direction, normal, p);
  f3 refined = ray_at(original, direction, refined_t);
  if (dot3(direction, normal) > 0.0f) { *back = offset_pt(refined, normal); *front = offset_pt(refined, neg3(normal)); }
  else                                { *back = offset_pt(refined, neg3(normal)); *front = offset_pt(refined, normal); }
}
/* utils_device.h:130-167 */
static float GTR1(float NDotH, float a) {
  if (a >= 1.f) return 1.f / ORC_PI;
  float a2 = a * a;
  float t = 1.f + (a2 - 1.f) * NDotH * NDotH;
  return (a2 - 1.0f) / (ORC_PI * logf(a2) * t);   /* AC6: logf of a per-material constant */
}
static float GTR2(float NDotH, float a) {
  float a2 = a * a;
  float t = 1.f + (a2 - 1.f) * NDotH * NDotH;
  return a2 / (ORC_PI * t * t);
}
static float GTR2Aniso(float NdotH, float HdotX, float HdotY, float ax, float ay) {
  return 1 / (ORC_PI * ax * ay * sqr(sqr(HdotX / ax) + sqr(HdotY / ay) + NdotH * NdotH));
}
static float schlickFresnel(float u) {
  float m = clampf(1.f - u, 0.f, 1.f);
  float m2 = m * m;
  return m2 * m2 * m;
}
static float smithGGgx(float NdotV, float alphaG) {
  float a = alphaG * alphaG;
  float b = NdotV * NdotV;
  return 1.f / (NdotV + sqrtf(a + b - a * b));
}
static float smithGGgxAniso(float NdotV, float VdotX, float VdotY, float ax, float ay) {
  return 1.0f / (NdotV + sqrtf(sqr(VdotX * ax) + sqr(VdotY * ay) + sqr(NdotV)));
}
/* utils_device.h:173-175; AC6 */
static inline float pow22(float x) { return (float)pow((double)x, (double)2.2f); }
static f3 srgb2lin(f3 v) { return mk3(pow22(v.x), pow22(v.y), pow22(v.z)); }

/* rtTex2D<float4>(id, u, v) with the sampler the reference creates (MinimalOptiX.cpp:449-474): repeat wrap,
 * normalized coordinates, bilinear filter.  CUDA texture units (which OptiX 5 uses) place texel centres at +0.5
 * and interpolate with weights quantised to 8 fractional bits. */
static inline int wrapi(int i, int n) { i %= n; return i < 0 ? i + n : i; }
static void tex2d(const OrcTexture* t, float u, float v, float out[4]) {
  const float x = (u - floorf(u)) * (float)t->width - 0.5f;
  const float y = (v - floorf(v)) * (float)t->height - 0.5f;
  const float fx = floorf(x), fy = floorf(y);
  const float ax = (float)(int)((x - fx) * 256.0f + 0.5f) * (1.0f / 256.0f);
  const float ay = (float)(int)((y - fy) * 256.0f + 0.5f) * (1.0f / 256.0f);
  const int i0 = wrapi((int)fx, t->width), i1 = wrapi((int)fx + 1, t->width);
  const int j0 = wrapi((int)fy, t->height), j1 = wrapi((int)fy + 1, t->height);
  const float* t00 = t->rgba + 4 * ((size_t)j0 * t->width + i0);
  const float* t10 = t->rgba + 4 * ((size_t)j0 * t->width + i1);
  const float* t01 = t->rgba + 4 * ((size_t)j1 * t->width + i0);
  const float* t11 = t->rgba + 4 * ((size_t)j1 * t->width + i1);
  for (int k = 0; k < 4; k++) {
    const float lo = t00[k] + ax * (t10[k] - t00[k]);
    const float hi = t01[k] + ax * (t11[k] - t01[k]);
    out[k] = lo + ay * (hi - lo);
  }
}
void orc_tex2d(const OrcTexture* t, float u, float v, float out[4]) { tex2d(t, u, v, out); }
/* utils_device.h:182-185 */
static float powerHeuristic(float a, float b) { float t = a * a; return t / (b * b + t); }

/* -------------------------------------------------------------- disney.h -- */
/* A1 cosine_sample_hemisphere */
static f3 cosine_sample_hemisphere(float u1, float u2) {
  const float r = sqrtf(u1);
  const float phi = (2.0f * ORC_PI) * u2;
  f3 p;
  float sinPhi, cosPhi;
  sincos_ac(phi, &sinPhi, &cosPhi);
  p.x = r * cosPhi;
  p.y = r * sinPhi;
  p.z = sqrtf(fmaxf(0.0f, 1.0f - p.x * p.x - p.y * p.y));
  return p;
}
/* disney.h:9-30 */
static void disney_sample(int32_t* seed, const OrcMaterial* m, f3 N, f3 V, f3* L, f3* H) {
  float diffuseRatio = 0.5f * (1.0f - m->metallic);
  Onb onb = onb_make(N);
  if (orc_rand(seed) < diffuseRatio) {
    float u1 = orc_rand(seed), u2 = orc_rand(seed);
    if (g_draw_order & 2) { float t_ = u1; u1 = u2; u2 = t_; }
    f3 l = cosine_sample_hemisphere(u1, u2);
    l = onb_inverse(&onb, l);
    *L = norm3(l);
    *H = norm3(add3(*L, V));
  } else {
    float a = fmaxf(0.001f, m->roughness);
    float phi = orc_rand(seed) * 2.0f * ORC_PI;
    float random = orc_rand(seed);
    float cosTheta = sqrtf((1.f - random) / (1.0f + (a * a - 1.f) * random));
    float sinTheta = sqrtf(1.0f - (cosTheta * cosTheta));
    float sinPhi, cosPhi;
    sincos_ac(phi, &sinPhi, &cosPhi);
    f3 h = mk3(sinTheta * cosPhi, sinTheta * sinPhi, cosTheta);
    h = onb_inverse(&onb, h);
    *L = norm3(sub3(scl3(h, 2.0f * dot3(V, h)), V));
    *H = norm3(h);
  }
}
/* disney.h:32-46 */
static float disney_pdf(const OrcMaterial* m, f3 N, f3 L, f3 V, f3 H) {
  (void)V;
  float diffuseRatio = 0.5f * (1.0f - m->metallic);
  float specularAlpha = fmaxf(0.001f, m->roughness);
  float clearcoatAlpha = lerpf(0.1f, 0.001f, m->clearcoatGloss);
  float specularRatio = 1.f - diffuseRatio;
  float cosTheta = fabsf(dot3(N, H));
  if (g_cos_short_tenth_ulp) cosTheta = (float)((double)cosTheta * (1.0 - 0.1 * (double)g_cos_short_tenth_ulp * 5.9604644775390625e-8));
  float pdfGTR1 = GTR1(cosTheta, clearcoatAlpha) * cosTheta;
  float pdfGTR2 = GTR2(cosTheta, specularAlpha) * cosTheta;
  float ratio = 1.0f / (1.0f + m->clearcoat);
  float pdfH = lerpf(pdfGTR1, pdfGTR2, ratio);
  float pdfL = pdfH / (4.0f * fabsf(dot3(L, H)));
  float pdfDiff = fabsf(dot3(N, L)) / ORC_PI;
  return diffuseRatio * pdfDiff + specularRatio * pdfL;
}
/* disney.h:48-91 */
static f3 disney_eval(const OrcMaterial* m, f3 baseColor, f3 N, f3 L, f3 V, f3 H) {
  Onb onb = onb_make(N);
  float NdotL = dot3(N, L), NdotV = dot3(N, V), NdotH = dot3(N, H), LdotH = dot3(L, H);
  f3 Cdlin = srgb2lin(baseColor);
  float Cdlum = dot3(Cdlin, mk3(0.3f, 0.6f, 0.1f));
  f3 Ctint = Cdlum > 0.f ? divs3(Cdlin, Cdlum) : mk3(1.f, 1.f, 1.f);
  f3 one = mk3(1.f, 1.f, 1.f);
  f3 Cspec0 = lerp3(scl3(lerp3(one, Ctint, m->specularTint), m->specular * 0.08f), Cdlin, m->metallic);
  f3 Csheen = lerp3(one, Ctint, m->sheenTint);

  float FL = schlickFresnel(NdotL);
  float FV = schlickFresnel(NdotV);
  float Fd90 = 0.5f + 2.f * LdotH * LdotH * m->roughness;
  float Fd = lerpf(1.f, Fd90, FL) * lerpf(1.f, Fd90, FV);

  float Fss90 = LdotH * LdotH * m->roughness;
  float Fss = lerpf(1.0f, Fss90, FL) * lerpf(1.0f, Fss90, FV);
  float ss = 1.25f * (Fss * (1.f / (NdotL + NdotV) - 0.5f) + 0.5f);

  float aspect = sqrtf(1 - m->anisotropic * 0.9f);
  float ax = fmaxf(.001f, sqr(m->roughness) / aspect);
  float ay = fmaxf(.001f, sqr(m->roughness) * aspect);
  f3 X = norm3(onb.tangent);
  f3 Y = norm3(cross3(N, X));
  float Ds = GTR2Aniso(NdotH, dot3(H, X), dot3(H, Y), ax, ay);
  float FH = schlickFresnel(LdotH);
  f3 Fs = lerp3(Cspec0, one, FH);
  float Gs = smithGGgxAniso(NdotL, dot3(L, X), dot3(L, Y), ax, ay) *
             smithGGgxAniso(NdotV, dot3(V, X), dot3(V, Y), ax, ay);
  f3 Fsheen = scl3(Csheen, FH * m->sheen);
  float Dr = GTR1(NdotH, lerpf(0.1f, 0.001f, m->clearcoatGloss));
  float Fr = lerpf(0.04f, 1.f, FH);
  float Gr = smithGGgx(NdotL, 0.25f) * smithGGgx(NdotV, 0.25f);
  /* ((1/pi)*lerp(Fd,ss,subsurface)*Cdlin + Fsheen)*(1-metallic) + Gs*Fs*Ds + 0.25*clearcoat*Gr*Fr*Dr */
  f3 diffuse = scl3(add3(scl3(Cdlin, (1.0f / ORC_PI) * lerpf(Fd, ss, m->subsurface)), Fsheen), 1.0f - m->metallic);
  f3 spec = scl3(scl3(Fs, Gs), Ds);
  float cc = 0.25f * m->clearcoat * Gr * Fr * Dr;
  return adds3(add3(diffuse, spec), cc);
}

/* ---------------------------------------------------------------------------------------------------------
 * "Exact arithmetic" variant of disneySample / disneyPdf / disneyEval: the same formulas (disney.h:9-91)
 * evaluated in binary64.  NOT the parity contract (the GPU computes in binary32, as the reference does); it
 * exists to tell apart, when the oracle is compared with the reference's demo images, what the FORMULAS give
 * from what binary32 rounding adds.  coffee.scene's Plastic_Orange has roughness 0.001, i.e. alpha^2 = 1e-6:
 * 1 + (alpha^2 - 1) cos^2(theta_h) is then computed from a cosine that is only known to 6e-8, and the
 * brightness of a light's reflection in that material depends on how every operation before it rounded
 * (DESIGN.md "coffee.png pin").  Enabled with orc_set_option("disney_binary64", 1). */
typedef struct { double x, y, z; } d3;
static inline d3 dmk(double x, double y, double z) { d3 r = { x, y, z }; return r; }
static inline d3 d_of(f3 a) { return dmk(a.x, a.y, a.z); }
static inline f3 f_of(d3 a) { return mk3((float)a.x, (float)a.y, (float)a.z); }
static inline d3 dadd(d3 a, d3 b) { return dmk(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline d3 dsub(d3 a, d3 b) { return dmk(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline d3 dscl(d3 a, double s) { return dmk(a.x * s, a.y * s, a.z * s); }
static inline double ddot(d3 a, d3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static inline d3 dcross(d3 a, d3 b) { return dmk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static inline d3 dnorm(d3 a) { return dscl(a, 1.0 / sqrt(ddot(a, a))); }
static inline double dlerp(double a, double b, double t) { return a + t * (b - a); }
static inline double dsqr(double x) { return x * x; }
static const double D_PI = (double)ORC_PI;
typedef struct { d3 tangent, binormal, normal; } OnbD;
static OnbD onb_make_d(d3 n) {
  OnbD o; o.normal = n;
  if (fabs(n.x) > fabs(n.z)) o.binormal = dmk(-n.y, n.x, 0.0); else o.binormal = dmk(0.0, -n.z, n.y);
  o.binormal = dnorm(o.binormal);
  o.tangent = dcross(o.binormal, o.normal);
  return o;
}
static d3 onb_inverse_d(const OnbD* o, d3 p) { return dadd(dadd(dscl(o->tangent, p.x), dscl(o->binormal, p.y)), dscl(o->normal, p.z)); }
static double schlick_d(double u) { double m = fmin(fmax(1.0 - u, 0.0), 1.0); double m2 = m * m; return m2 * m2 * m; }
static double GTR1_d(double c, double a) { if (a >= 1.0) return 1.0 / D_PI; double a2 = a * a; return (a2 - 1.0) / (D_PI * log(a2) * (1.0 + (a2 - 1.0) * c * c)); }
static double GTR2_d(double c, double a) { double a2 = a * a, t = 1.0 + (a2 - 1.0) * c * c; return a2 / (D_PI * t * t); }
static double smithG_d(double nv, double ag) { double a = ag * ag, b = nv * nv; return 1.0 / (nv + sqrt(a + b - a * b)); }
static double smithGA_d(double nv, double vx, double vy, double ax, double ay) { return 1.0 / (nv + sqrt(dsqr(vx * ax) + dsqr(vy * ay) + dsqr(nv))); }
/* same random draws, in the same order, as disney_sample */
static void disney_sample_d(int32_t* seed, const OrcMaterial* m, d3 N, d3 V, d3* L, d3* H) {
  double diffuseRatio = 0.5 * (1.0 - (double)m->metallic);
  OnbD onb = onb_make_d(N);
  if ((double)orc_rand(seed) < diffuseRatio) {
    double u1 = orc_rand(seed), u2 = orc_rand(seed);
    double r = sqrt(u1), phi = 2.0 * D_PI * u2;
    d3 l = dmk(r * cos(phi), r * sin(phi), 0.0);
    l.z = sqrt(fmax(0.0, 1.0 - l.x * l.x - l.y * l.y));
    *L = dnorm(onb_inverse_d(&onb, l));
    *H = dnorm(dadd(*L, V));
  } else {
    double a = fmax(0.001, (double)m->roughness);
    double phi = (double)orc_rand(seed) * 2.0 * D_PI;
    double random = orc_rand(seed);
    double cosTheta = sqrt((1.0 - random) / (1.0 + (a * a - 1.0) * random));
    double sinTheta = sqrt(1.0 - cosTheta * cosTheta);
    d3 h = onb_inverse_d(&onb, dmk(sinTheta * cos(phi), sinTheta * sin(phi), cosTheta));
    *L = dnorm(dsub(dscl(h, 2.0 * ddot(V, h)), V));
    *H = dnorm(h);
  }
}
static double disney_pdf_d(const OrcMaterial* m, d3 N, d3 L, d3 H) {
  double diffuseRatio = 0.5 * (1.0 - (double)m->metallic);
  double c = fabs(ddot(N, H));
  double pdfH = dlerp(GTR1_d(c, dlerp(0.1, 0.001, m->clearcoatGloss)) * c, GTR2_d(c, fmax(0.001, (double)m->roughness)) * c, 1.0 / (1.0 + (double)m->clearcoat));
  return diffuseRatio * fabs(ddot(N, L)) / D_PI + (1.0 - diffuseRatio) * pdfH / (4.0 * fabs(ddot(L, H)));
}
static d3 disney_eval_d(const OrcMaterial* m, f3 baseColor, d3 N, d3 L, d3 V, d3 H) {
  OnbD onb = onb_make_d(N);
  double NdotL = ddot(N, L), NdotV = ddot(N, V), NdotH = ddot(N, H), LdotH = ddot(L, H);
  d3 Cdlin = dmk(pow(baseColor.x, (double)2.2f), pow(baseColor.y, (double)2.2f), pow(baseColor.z, (double)2.2f));
  double Cdlum = 0.3 * Cdlin.x + 0.6 * Cdlin.y + 0.1 * Cdlin.z;
  d3 one = dmk(1, 1, 1);
  d3 Ctint = Cdlum > 0 ? dscl(Cdlin, 1.0 / Cdlum) : one;
  d3 t0 = dscl(dadd(one, dscl(dsub(Ctint, one), m->specularTint)), (double)m->specular * 0.08);
  d3 Cspec0 = dadd(t0, dscl(dsub(Cdlin, t0), m->metallic));
  d3 Csheen = dadd(one, dscl(dsub(Ctint, one), m->sheenTint));
  double FL = schlick_d(NdotL), FV = schlick_d(NdotV), r = m->roughness;
  double Fd90 = 0.5 + 2.0 * LdotH * LdotH * r;
  double Fd = dlerp(1.0, Fd90, FL) * dlerp(1.0, Fd90, FV);
  double Fss90 = LdotH * LdotH * r;
  double Fss = dlerp(1.0, Fss90, FL) * dlerp(1.0, Fss90, FV);
  double ss = 1.25 * (Fss * (1.0 / (NdotL + NdotV) - 0.5) + 0.5);
  double aspect = sqrt(1.0 - (double)m->anisotropic * 0.9);
  double ax = fmax(.001, r * r / aspect), ay = fmax(.001, r * r * aspect);
  d3 X = dnorm(onb.tangent), Y = dnorm(dcross(N, X));
  double Ds = 1.0 / (D_PI * ax * ay * dsqr(dsqr(ddot(H, X) / ax) + dsqr(ddot(H, Y) / ay) + NdotH * NdotH));
  double FH = schlick_d(LdotH);
  d3 Fs = dadd(Cspec0, dscl(dsub(one, Cspec0), FH));
  double Gs = smithGA_d(NdotL, ddot(L, X), ddot(L, Y), ax, ay) * smithGA_d(NdotV, ddot(V, X), ddot(V, Y), ax, ay);
  d3 Fsheen = dscl(Csheen, FH * (double)m->sheen);
  double Dr = GTR1_d(NdotH, dlerp(0.1, 0.001, m->clearcoatGloss));
  double Fr = dlerp(0.04, 1.0, FH);
  double Gr = smithG_d(NdotL, 0.25) * smithG_d(NdotV, 0.25);
  d3 diffuse = dscl(dadd(dscl(Cdlin, (1.0 / D_PI) * dlerp(Fd, ss, m->subsurface)), Fsheen), 1.0 - (double)m->metallic);
  d3 spec = dscl(Fs, Gs * Ds);
  double cc = 0.25 * (double)m->clearcoat * Gr * Fr * Dr;
  return dmk(diffuse.x + spec.x + cc, diffuse.y + spec.y + cc, diffuse.z + spec.z + cc);
}
int orc_set_option(const char* name, int value) {
  if (!strcmp(name, "disney_binary64")) { g_disney_binary64 = value != 0; return 0; }
  if (!strcmp(name, "indirect_scale_pct")) { g_indirect_scale_pct = value; return 0; }
  if (!strcmp(name, "indirect_depth1_off")) { g_indirect_depth1_off = value != 0; return 0; }
  if (!strcmp(name, "draw_order")) { g_draw_order = value; return 0; }
  if (!strcmp(name, "noshadow_first")) { g_noshadow_first = value; return 0; }
  if (!strcmp(name, "noshadow_last")) { g_noshadow_last = value; return 0; }
  if (!strcmp(name, "shadow_any_opaque_blocks")) { g_shadow_any_opaque_blocks = value != 0; return 0; }
  if (!strcmp(name, "cos_short_tenth_ulp")) { g_cos_short_tenth_ulp = value; return 0; }
  return -1;
}

float orc_disney_pdf(const OrcMaterial* m, const float N[3], const float L[3], const float V[3], const float H[3]) {
  return disney_pdf(m, ld3(N), ld3(L), ld3(V), ld3(H));
}
void orc_disney_eval(const OrcMaterial* m, const float base[3], const float N[3], const float L[3],
                     const float V[3], const float H[3], float out[3]) {
  st3(out, disney_eval(m, ld3(base), ld3(N), ld3(L), ld3(V), ld3(H)));
}
void orc_disney_sample(int32_t* seed, const OrcMaterial* m, const float N[3], const float V[3], float L[3], float H[3]) {
  f3 l, h; disney_sample(seed, m, ld3(N), ld3(V), &l, &h); st3(L, l); st3(H, h);
}
int orc_refract(float r[3], const float i[3], const float n[3], float ior) {
  f3 rr; int ok = refract3(&rr, ld3(i), ld3(n), ior); st3(r, rr); return ok;
}

/* --------------------------------------------------------- intersection -- */
/* A1 intersect_triangle (== intersect_triangle_branchless) */
static int tri_test(f3 o, f3 d, float tmin, float tmax, f3 p0, f3 p1, f3 p2,
                    f3* n, float* t, float* beta, float* gamma) {
  const f3 e0 = sub3(p1, p0);
  const f3 e1 = sub3(p0, p2);
  *n = cross3(e1, e0);
  const f3 e2 = scl3(sub3(p0, o), 1.0f / dot3(*n, d));
  const f3 i = cross3(d, e2);
  *beta = dot3(i, e1);
  *gamma = dot3(i, e0);
  *t = dot3(*n, e2);
  return (*t < tmax) & (*t > tmin) & (*beta >= 0.0f) & (*gamma >= 0.0f) & (*beta + *gamma <= 1.0f);
}
int orc_intersect_triangle(const float o[3], const float d[3], float tmin, float tmax,
                           const float p0[3], const float p1[3], const float p2[3],
                           float n[3], float* t, float* beta, float* gamma) {
  f3 nn; int r = tri_test(ld3(o), ld3(d), tmin, tmax, ld3(p0), ld3(p1), ld3(p2), &nn, t, beta, gamma);
  st3(n, nn); return r;
}

/* Independent triangle BVH (median split, <=4 tris per leaf). Boxes are padded
 * and the slab test is slack so that culling can never reject a triangle the
 * exact test would accept: results equal brute force (tests check this). */
typedef struct { float bmin[3], bmax[3]; int32_t left, right, first, count; } BNode;
typedef struct { BNode* nodes; int32_t nNodes; int32_t* order; } TriBVH;

static const float* g_centroids;   /* qsort context (build is single threaded) */
static int g_axis;
static int cmp_centroid(const void* a, const void* b) {
  float ca = g_centroids[3 * (*(const int32_t*)a) + g_axis], cb = g_centroids[3 * (*(const int32_t*)b) + g_axis];
  if (ca < cb) return -1;
  if (ca > cb) return 1;
  int32_t ia = *(const int32_t*)a, ib = *(const int32_t*)b;
  return (ia > ib) - (ia < ib);
}
static int32_t bvh_build_rec(TriBVH* bvh, const float* tmin3, const float* tmax3, int32_t first, int32_t count) {
  int32_t id = bvh->nNodes++;
  BNode* nd = &bvh->nodes[id];
  float cmin[3] = { 1e37f, 1e37f, 1e37f }, cmax[3] = { -1e37f, -1e37f, -1e37f };
  for (int k = 0; k < 3; k++) { nd->bmin[k] = 1e37f; nd->bmax[k] = -1e37f; }
  for (int32_t i = first; i < first + count; i++) {
    int32_t t = bvh->order[i];
    for (int k = 0; k < 3; k++) {
      nd->bmin[k] = fminf(nd->bmin[k], tmin3[3 * t + k]);
      nd->bmax[k] = fmaxf(nd->bmax[k], tmax3[3 * t + k]);
      float c = g_centroids[3 * t + k];
      cmin[k] = fminf(cmin[k], c); cmax[k] = fmaxf(cmax[k], c);
    }
  }
  nd->first = first; nd->count = count; nd->left = nd->right = -1;
  if (count <= 4) return id;
  int axis = 0; float ext = cmax[0] - cmin[0];
  for (int k = 1; k < 3; k++) if (cmax[k] - cmin[k] > ext) { ext = cmax[k] - cmin[k]; axis = k; }
  g_axis = axis;
  qsort(bvh->order + first, (size_t)count, sizeof(int32_t), cmp_centroid);
  int32_t half = count / 2;
  int32_t l = bvh_build_rec(bvh, tmin3, tmax3, first, half);
  int32_t r = bvh_build_rec(bvh, tmin3, tmax3, first + half, count - half);
  nd = &bvh->nodes[id];
  nd->left = l; nd->right = r; nd->count = 0;
  return id;
}
static TriBVH* bvh_build(const OrcScene* sc) {
  int32_t n = sc->nFaces;
  TriBVH* bvh = (TriBVH*)calloc(1, sizeof(TriBVH));
  bvh->nodes = (BNode*)malloc(sizeof(BNode) * (size_t)(2 * n + 1));
  bvh->order = (int32_t*)malloc(sizeof(int32_t) * (size_t)n);
  float* tmin3 = (float*)malloc(sizeof(float) * 3 * (size_t)n);
  float* tmax3 = (float*)malloc(sizeof(float) * 3 * (size_t)n);
  float* cen = (float*)malloc(sizeof(float) * 3 * (size_t)n);
  float smin[3] = { 1e37f, 1e37f, 1e37f }, smax[3] = { -1e37f, -1e37f, -1e37f };
  for (int32_t t = 0; t < n; t++) {
    bvh->order[t] = t;
    for (int k = 0; k < 3; k++) {
      float a = sc->positions[3 * sc->vIdx[3 * t + 0] + k];
      float b = sc->positions[3 * sc->vIdx[3 * t + 1] + k];
      float c = sc->positions[3 * sc->vIdx[3 * t + 2] + k];
      tmin3[3 * t + k] = fminf(fminf(a, b), c);
      tmax3[3 * t + k] = fmaxf(fmaxf(a, b), c);
      cen[3 * t + k] = (tmin3[3 * t + k] + tmax3[3 * t + k]) * 0.5f;
      smin[k] = fminf(smin[k], tmin3[3 * t + k]); smax[k] = fmaxf(smax[k], tmax3[3 * t + k]);
    }
  }
  /* pad every triangle box by a scene-relative slack */
  float diag = fmaxf(fmaxf(smax[0] - smin[0], smax[1] - smin[1]), smax[2] - smin[2]);
  float pad = 1e-5f * diag + 1e-30f;
  for (int32_t i = 0; i < 3 * n; i++) { tmin3[i] -= pad + 1e-6f * fabsf(tmin3[i]); tmax3[i] += pad + 1e-6f * fabsf(tmax3[i]); }
  g_centroids = cen;
  if (n > 0) bvh_build_rec(bvh, tmin3, tmax3, 0, n);
  free(tmin3); free(tmax3); free(cen);
  return bvh;
}
static void bvh_free(TriBVH* b) { if (!b) return; free(b->nodes); free(b->order); free(b); }

typedef struct {
  float t; int32_t prim; int32_t mat;
  f3 geoNormal, shadingNormal, frontHitPoint, backHitPoint;
  float texu, texv;     /* texcoord attribute (Geometry.cu:37, 141-148) */
} Hit;

typedef struct {
  const OrcScene* sc;
  const TriBVH* bvh;
  OrcStats st;
  int32_t maxDepth;     /* analysis: deepest payload.depth a radiance rtTrace of the current sample was issued with */
  f3 lastRaw;           /* analysis: the last sample's colour before the per-sample clamp */
} Ctx;

/* rtPotentialIntersection restated with a deterministic equal-t rule
 * (SURVEY A2 divergence D5): nearer t wins; at exactly equal t the lower
 * primitive id wins.  Primitive ids: spheres, then quads, then triangles. */
static inline int potential(float t, int32_t prim, float tmin, float tbest, int32_t bestPrim) {
  return ((t > tmin) & (t < tbest)) | ((t == tbest) & (bestPrim >= 0) & (prim < bestPrim));
}

/* Geometry.cu:18-55 (root selection only; attributes are filled for the winner) */
static int sphere_roots(const OrcSphere* s, f3 o, f3 d, float* t1, float* t2) {
  f3 oc = sub3(o, ld3(s->center));
  float b = dot3(d, oc);
  float c = dot3(oc, oc) - s->radius * s->radius;
  float disc = b * b - c;
  if (disc < 0) return 0;
  float sq = sqrtf(disc);
  *t1 = -b - sq; *t2 = -b + sq;
  return 1;
}
/* Geometry.cu:70-91 */
static int quad_test(const OrcQuad* q, f3 o, f3 d, float tmin, float tmax, float* tOut) {
  f3 n = mk3(q->plane[0], q->plane[1], q->plane[2]);
  float dt = dot3(d, n);
  float t = (q->plane[3] - dot3(n, o)) / dt;
  if (t > tmin && t < tmax) {
    f3 p = ray_at(o, d, t);
    f3 vi = sub3(p, ld3(q->anchor));
    float a1 = dot3(ld3(q->v1), vi);
    if (a1 >= 0 && a1 <= 1) {
      float a2 = dot3(ld3(q->v2), vi);
      if (a2 >= 0 && a2 <= 1) { *tOut = t; return 1; }
    }
  }
  return 0;
}
static inline f3 vert(const OrcScene* sc, int32_t i) { return ld3(sc->positions + 3 * (size_t)i); }

static inline int box_hit(const BNode* nd, f3 o, f3 inv, float tmin, float tmax) {
  float t0x = (nd->bmin[0] - o.x) * inv.x, t1x = (nd->bmax[0] - o.x) * inv.x;
  float t0y = (nd->bmin[1] - o.y) * inv.y, t1y = (nd->bmax[1] - o.y) * inv.y;
  float t0z = (nd->bmin[2] - o.z) * inv.z, t1z = (nd->bmax[2] - o.z) * inv.z;
  float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fmaxf(fminf(t0z, t1z), tmin));
  float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fminf(fmaxf(t0z, t1z), tmax));
  return tn <= tf * 1.0000005f + 1e-30f;
}

/* rtTrace nearest-hit search (A1), ray type radiance.  Returns 1 on hit. */
static int find_closest(Ctx* cx, f3 o, f3 d, float tmin, float tmax, Hit* hit) {
  const OrcScene* sc = cx->sc;
  float best = tmax; int32_t bestPrim = -1; int bestRoot = 0;
  for (int32_t i = 0; i < sc->nSpheres; i++) {
    float t1, t2;
    if (!sphere_roots(&sc->spheres[i], o, d, &t1, &t2)) continue;
    if (potential(t1, i, tmin, best, bestPrim)) { best = t1; bestPrim = i; bestRoot = 1; }
    else if (potential(t2, i, tmin, best, bestPrim)) { best = t2; bestPrim = i; bestRoot = 2; }
  }
  for (int32_t i = 0; i < sc->nQuads; i++) {
    float t; int32_t id = sc->nSpheres + i;
    /* Geometry.cu:74 tests against ray.tmax then rtPotentialIntersection */
    if (quad_test(&sc->quads[i], o, d, tmin, tmax, &t) && potential(t, id, tmin, best, bestPrim)) { best = t; bestPrim = id; }
  }
  const int32_t triBase = sc->nSpheres + sc->nQuads;
  float bBeta = 0, bGamma = 0; f3 bN = mk3(0, 0, 0);
  if (sc->nFaces > 0) {
    if (sc->bruteForceTris || !cx->bvh) {
      for (int32_t f = 0; f < sc->nFaces; f++) {
        f3 n; float t, be, ga;
        if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga)
            && potential(t, triBase + f, tmin, best, bestPrim)) { best = t; bestPrim = triBase + f; bBeta = be; bGamma = ga; bN = n; }
      }
    } else {
      const TriBVH* bvh = cx->bvh;
      f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      int32_t stack[128]; int sp = 0; stack[sp++] = 0;
      while (sp > 0) {
        const BNode* nd = &bvh->nodes[stack[--sp]];
        if (!box_hit(nd, o, inv, tmin, best)) continue;
        if (nd->left < 0) {
          for (int32_t k = nd->first; k < nd->first + nd->count; k++) {
            int32_t f = bvh->order[k];
            f3 n; float t, be, ga;
            if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga)
                && potential(t, triBase + f, tmin, best, bestPrim)) { best = t; bestPrim = triBase + f; bBeta = be; bGamma = ga; bN = n; }
          }
        } else { stack[sp++] = nd->left; stack[sp++] = nd->right; }
      }
    }
  }
  if (bestPrim < 0) return 0;
  hit->t = best; hit->prim = bestPrim; hit->texu = 0.f; hit->texv = 0.f;
  if (bestPrim < sc->nSpheres) {                       /* Geometry.cu:30-53 */
    const OrcSphere* s = &sc->spheres[bestPrim];
    (void)bestRoot;
    f3 p = ray_at(o, d, best);
    hit->geoNormal = norm3(sub3(p, ld3(s->center)));
    hit->shadingNormal = hit->geoNormal;
    hit->frontHitPoint = p; hit->backHitPoint = p;
    hit->mat = s->mat;
  } else if (bestPrim < triBase) {                     /* Geometry.cu:81-86 */
    const OrcQuad* q = &sc->quads[bestPrim - sc->nSpheres];
    f3 n = mk3(q->plane[0], q->plane[1], q->plane[2]);
    hit->geoNormal = n; hit->shadingNormal = n;
    hit->frontHitPoint = ray_at(o, d, best); hit->backHitPoint = hit->frontHitPoint;
    hit->mat = q->mat;
  } else {                                             /* Geometry.cu:134-157 */
    int32_t f = bestPrim - triBase;
    hit->geoNormal = norm3(bN);
    const int32_t* ni = sc->nIdx + 3 * (size_t)f;
    if (sc->nNorms == 0 || ni[0] < 0 || ni[1] < 0 || ni[2] < 0) {
      hit->shadingNormal = hit->geoNormal;
    } else {
      f3 n0 = ld3(sc->normals + 3 * (size_t)ni[0]), n1 = ld3(sc->normals + 3 * (size_t)ni[1]), n2 = ld3(sc->normals + 3 * (size_t)ni[2]);
      hit->shadingNormal = norm3(add3(add3(scl3(n1, bBeta), scl3(n2, bGamma)), scl3(n0, 1.f - bBeta - bGamma)));
    }
    const int32_t* ti = sc->tIdx ? sc->tIdx + 3 * (size_t)f : NULL;
    if (sc->nUVs > 0 && ti && ti[0] >= 0 && ti[1] >= 0 && ti[2] >= 0) {            /* Geometry.cu:141-148 */
      const float* t0 = sc->texcoords + 2 * (size_t)ti[0]; const float* t1 = sc->texcoords + 2 * (size_t)ti[1];
      const float* t2 = sc->texcoords + 2 * (size_t)ti[2];
      const float w0 = 1.0f - bBeta - bGamma;
      hit->texu = (t1[0] * bBeta + t2[0] * bGamma) + t0[0] * w0;
      hit->texv = (t1[1] * bBeta + t2[1] * bGamma) + t0[1] * w0;
    }
    refine_hitpoint(ray_at(o, d, best), d, hit->geoNormal, vert(sc, sc->vIdx[3 * f]), &hit->backHitPoint, &hit->frontHitPoint);
    hit->mat = sc->faceMat[f];
  }
  return 1;
}

int orc_closest_hit(const OrcScene* sc, const float org[3], const float dir[3], float tmin, float tmax, float* tHit) {
  Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc;
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
  cx.bvh = bvh;
  Hit h; int r = find_closest(&cx, ld3(org), ld3(dir), tmin, tmax, &h);
  bvh_free(bvh);
  if (!r) return -1;
  if (tHit) *tHit = h.t;
  return h.prim;
}

/* n nearest-hit queries against one tree: rays = n x {o.xyz, d.xyz, tmin, tmax} (the layout of moptix_debug_trace) */
int orc_closest_hit_batch(const OrcScene* sc, const float* rays, int n, int32_t* outPrim, float* outT) {
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
#pragma omp parallel for schedule(dynamic, 64)
  for (int i = 0; i < n; i++) {
    Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc; cx.bvh = bvh;
    const float* r = rays + 8 * (size_t)i;
    Hit h;
    if (find_closest(&cx, ld3(r), ld3(r + 3), r[6], r[7], &h)) { outPrim[i] = h.prim; outT[i] = h.t; }
    else { outPrim[i] = -1; outT[i] = 0.f; }
  }
  bvh_free(bvh);
  return 0;
}

/* Shadow ray (ray type 1): Material.cu:187-193 + disneyAnyHit :225-232.
 *
 * OptiX semantics: rtReportIntersection runs the any-hit program of the instance's material for the ray type; a
 * program that neither calls rtIgnoreIntersection nor rtTerminateRay ACCEPTS the hit, and the ray's tmax becomes that t --
 * nothing farther along the ray is reported any more.  disneyAnyHit terminates on an opaque surface (attenuation = 0) and does
 * neither on a GLASS surface (attenuation *= color).  With a front-to-back traversal the shadow ray is therefore decided by the
 * NEAREST surface that has the program: opaque -> (0,0,0); glass -> that surface's colour, and whatever lies behind the glass,
 * opaque or not, never blocks.  (In OptiX proper the order is the BVH's and the outcome can differ from ray to ray -- SURVEY D5;
 * "nearest by (t, primitive id)" is the deterministic definition.)  Instances without the program (lights, lambertian / metal /
 * glass spheres and quads) are not there for a shadow ray.
 *
 * Rounds 1-2 used SURVEY A2's simpler rule (an opaque surface anywhere on the segment blocks); the two only differ when a Disney
 * GLASS surface is the first thing on the segment and something opaque follows.  The reference's demo/coffee.png shows which one
 * the reference does: the floor round the machine is lit THROUGH the glass pot past the lid and the body above it. */
static inline int shadow_apply(const OrcScene* sc, int32_t mat, f3* att) {
  const OrcMaterial* m = &sc->materials[mat];
  if (m->kind != ORC_DISNEY) return 0;
  if (m->brdfType == ORC_BRDF_GLASS) { *att = mul3(*att, ld3(m->color)); return 0; }
  if (mat >= g_noshadow_first && mat <= g_noshadow_last) return 0;      /* analysis switch, off by default */
  *att = mk3(0.f, 0.f, 0.f);
  return 1; /* rtTerminateRay */
}
/* verdict of one candidate: a primitive whose material has the shadow any-hit program, intersected at t */
static inline void shadow_candidate(const OrcScene* sc, int32_t mat, float t, int32_t prim, float tmin, float* best, int32_t* bestPrim, f3* att) {
  const OrcMaterial* m = &sc->materials[mat];
  if (m->kind != ORC_DISNEY) return;
  if (potential(t, prim, tmin, *best, *bestPrim)) {
    *best = t; *bestPrim = prim;
    *att = (m->brdfType == ORC_BRDF_GLASS) ? ld3(m->color) : mk3(0.f, 0.f, 0.f);
  }
}
/* the nearest (t, primitive id) any-hit surface in (tmin, tmax) decides */
static f3 shadow_nearest(Ctx* cx, f3 o, f3 d, float tmin, float tmax) {
  const OrcScene* sc = cx->sc;
  f3 att = mk3(1.f, 1.f, 1.f);
  float best = tmax; int32_t bestPrim = -1;
  for (int32_t i = 0; i < sc->nSpheres; i++) {
    float t1, t2;
    if (!sphere_roots(&sc->spheres[i], o, d, &t1, &t2)) continue;
    shadow_candidate(sc, sc->spheres[i].mat, t1, i, tmin, &best, &bestPrim, &att);
    shadow_candidate(sc, sc->spheres[i].mat, t2, i, tmin, &best, &bestPrim, &att);
  }
  for (int32_t i = 0; i < sc->nQuads; i++) {
    float t;
    if (quad_test(&sc->quads[i], o, d, tmin, tmax, &t)) shadow_candidate(sc, sc->quads[i].mat, t, sc->nSpheres + i, tmin, &best, &bestPrim, &att);
  }
  const int32_t triBase = sc->nSpheres + sc->nQuads;
  if (sc->nFaces > 0) {
    if (sc->bruteForceTris || !cx->bvh) {
      for (int32_t f = 0; f < sc->nFaces; f++) {
        f3 n; float t, be, ga;
        if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga))
          shadow_candidate(sc, sc->faceMat[f], t, triBase + f, tmin, &best, &bestPrim, &att);
      }
    } else {
      const TriBVH* bvh = cx->bvh;
      f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      int32_t stack[128]; int sp = 0; stack[sp++] = 0;
      while (sp > 0) {
        const BNode* nd = &bvh->nodes[stack[--sp]];
        if (!box_hit(nd, o, inv, tmin, best)) continue;
        if (nd->left < 0) {
          for (int32_t k = nd->first; k < nd->first + nd->count; k++) {
            int32_t f = bvh->order[k];
            f3 n; float t, be, ga;
            if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga))
              shadow_candidate(sc, sc->faceMat[f], t, triBase + f, tmin, &best, &bestPrim, &att);
          }
        } else { stack[sp++] = nd->left; stack[sp++] = nd->right; }
      }
    }
  }
  return att;
}
static f3 shadow_attenuation(Ctx* cx, f3 o, f3 d, float tmin, float tmax) {
  const OrcScene* sc = cx->sc;
  f3 att = mk3(1.f, 1.f, 1.f);
  int anyGlass = 0;
  for (int32_t i = 0; i < sc->nMaterials; i++) if (sc->materials[i].kind == ORC_DISNEY && sc->materials[i].brdfType == ORC_BRDF_GLASS) anyGlass = 1;
  if (anyGlass && !g_shadow_any_opaque_blocks) return shadow_nearest(cx, o, d, tmin, tmax);
  /* no Disney GLASS material in the scene: "the nearest any-hit surface is opaque" == "some opaque surface is on the segment" */
  for (int32_t i = 0; i < sc->nSpheres; i++) {
    float t1, t2;
    if (sc->materials[sc->spheres[i].mat].kind != ORC_DISNEY) continue;
    if (!sphere_roots(&sc->spheres[i], o, d, &t1, &t2)) continue;
    if ((t1 > tmin && t1 < tmax) || (t2 > tmin && t2 < tmax)) if (shadow_apply(sc, sc->spheres[i].mat, &att)) return att;
  }
  for (int32_t i = 0; i < sc->nQuads; i++) {
    float t;
    if (sc->materials[sc->quads[i].mat].kind != ORC_DISNEY) continue;
    if (quad_test(&sc->quads[i], o, d, tmin, tmax, &t)) if (shadow_apply(sc, sc->quads[i].mat, &att)) return att;
  }
  if (sc->nFaces > 0) {
    if (sc->bruteForceTris || !cx->bvh) {
      for (int32_t f = 0; f < sc->nFaces; f++) {
        f3 n; float t, be, ga;
        if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga))
          if (shadow_apply(sc, sc->faceMat[f], &att)) return att;
      }
    } else {
      const TriBVH* bvh = cx->bvh;
      f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
      int32_t stack[128]; int sp = 0; stack[sp++] = 0;
      while (sp > 0) {
        const BNode* nd = &bvh->nodes[stack[--sp]];
        if (!box_hit(nd, o, inv, tmin, tmax)) continue;
        if (nd->left < 0) {
          for (int32_t k = nd->first; k < nd->first + nd->count; k++) {
            int32_t f = bvh->order[k];
            f3 n; float t, be, ga;
            if (tri_test(o, d, tmin, tmax, vert(sc, sc->vIdx[3 * f]), vert(sc, sc->vIdx[3 * f + 1]), vert(sc, sc->vIdx[3 * f + 2]), &n, &t, &be, &ga))
              if (shadow_apply(sc, sc->faceMat[f], &att)) return att;
          }
        } else { stack[sp++] = nd->left; stack[sp++] = nd->right; }
      }
    }
  }
  return att;
}

/* ------------------------------------------------------- material programs -- */
typedef struct { f3 color; int32_t depth; int32_t randSeed; } Payload;   /* Structures.h:5-10 */

static void trace_radiance(Ctx* cx, f3 o, f3 d, float tmin, float tmax, Payload* pld);

/* utils_device.h:192-198 folkPayload */
static Payload fork_payload(const Payload* parent) {
  Payload c; c.depth = parent->depth + 1; c.color = mk3(1.f, 1.f, 1.f);
  c.randSeed = (int32_t)orc_tea16((uint32_t)parent->randSeed, (uint32_t)c.depth);
  return c;
}
static inline int absorbed(const OrcScene* sc, const Payload* p) {   /* Material.cu:29,50,73,119 */
  return (p->depth > sc->rayMaxDepth) || (len3(p->color) < sc->rayMinIntensity);
}

/* Material.cu:28-43 */
static void prog_lambertian(Ctx* cx, const OrcMaterial* m, f3 o, f3 d, const Hit* h, Payload* p) {
  if (absorbed(cx->sc, p)) { cx->st.depthCapped++; p->color = mk3(0.f, 0.f, 0.f); return; }
  f3 no = ray_at(o, d, h->t);
  f3 nd = norm3(add3(h->geoNormal, rand_in_unit_sphere(&p->randSeed)));
  Payload c = fork_payload(p);
  cx->st.bounceRays++;
  trace_radiance(cx, no, nd, cx->sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &c);
  p->color = mul3(c.color, ld3(m->albedo));
}
/* Material.cu:49-66 */
static void prog_metal(Ctx* cx, const OrcMaterial* m, f3 o, f3 d, const Hit* h, Payload* p) {
  if (absorbed(cx->sc, p)) { cx->st.depthCapped++; p->color = mk3(0.f, 0.f, 0.f); return; }
  f3 no = ray_at(o, d, h->t);
  f3 nd = norm3(add3(reflect3(d, h->geoNormal), scl3(rand_in_unit_sphere(&p->randSeed), m->fuzz)));
  Payload c = fork_payload(p);
  cx->st.bounceRays++;
  trace_radiance(cx, no, nd, cx->sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &c);
  p->color = mul3(ld3(m->albedo), c.color);
}
/* Material.cu:72-110 (glass) and :134-168 (disney GLASS branch) share this body */
static void glass_body(Ctx* cx, float ior, f3 tint, f3 d, const Hit* h, Payload* p) {
  f3 normal = h->shadingNormal;
  float cosThetaI = -dot3(d, normal);
  float refIdx;
  if (cosThetaI > 0.f) { refIdx = ior; }
  else { refIdx = 1.f / ior; cosThetaI = -cosThetaI; normal = neg3(normal); }
  f3 refracted;
  int totalReflection = !refract3(&refracted, d, normal, refIdx);
  float cosThetaT = -dot3(normal, refracted);
  float reflectProb = totalReflection ? 1.f : fresnel(cosThetaI, cosThetaT, refIdx);
  Payload c = fork_payload(p);                  /* fork BEFORE the draw: Material.cu:100-101 */
  f3 no, nd;
  if (orc_rand(&p->randSeed) < reflectProb) { no = h->frontHitPoint; nd = reflect3(d, normal); }
  else { no = h->backHitPoint; nd = refracted; }
  cx->st.bounceRays++;
  trace_radiance(cx, no, nd, cx->sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &c);
  p->color = mul3(c.color, tint);
}
static void prog_glass(Ctx* cx, const OrcMaterial* m, f3 d, const Hit* h, Payload* p) {
  if (absorbed(cx->sc, p)) { cx->st.depthCapped++; p->color = mk3(0.f, 0.f, 0.f); return; }
  glass_body(cx, m->refIdx, ld3(m->albedo), d, h, p);
}
/* Material.cu:118-223 */
static void prog_disney(Ctx* cx, const OrcMaterial* m, f3 d, const Hit* h, Payload* p) {
  const OrcScene* sc = cx->sc;
  if (absorbed(sc, p)) { cx->st.depthCapped++; p->color = mk3(0.f, 0.f, 0.f); return; }
  f3 N = faceforward3(h->shadingNormal, neg3(d), h->geoNormal);
  f3 V = neg3(d);
  f3 L, H;
  f3 baseColor = ld3(m->color);
  if (m->albedoID != 0 && m->albedoID <= sc->nTextures) {      /* Material.cu:128-132 */
    float tc[4];
    tex2d(&sc->textures[m->albedoID - 1], h->texu, h->texv, tc);
    baseColor = mk3(tc[0], tc[1], tc[2]);
  }
  if (m->brdfType == ORC_BRDF_GLASS) { glass_body(cx, 1.45f, baseColor, d, h, p); return; }
  const d3 Nd = dnorm(d_of(N)), Vd = dnorm(d_of(V));   /* binary64 analysis mode: unit vectors to 1e-16, not 6e-8 */

  f3 direct = mk3(0.f, 0.f, 0.f);
  for (int32_t i = 0; i < sc->nLights; ++i) {
    const OrcLight* light = &sc->lights[i];
    f3 pointOnLight, normalOnLight;
    if (light->shape == ORC_LIGHT_SPHERE) {
      pointOnLight = add3(ld3(light->position), scl3(rand_in_unit_sphere(&p->randSeed), light->radius));
      normalOnLight = norm3(sub3(pointOnLight, ld3(light->position)));
    } else {
      float r1 = orc_rand(&p->randSeed); float r2 = orc_rand(&p->randSeed);
      if (g_draw_order & 1) { float t_ = r1; r1 = r2; r2 = t_; }
      pointOnLight = add3(add3(ld3(light->position), scl3(ld3(light->u), r1)), scl3(ld3(light->v), r2));
      normalOnLight = norm3(ld3(light->normal));
    }
    L = sub3(pointOnLight, h->frontHitPoint);
    float lightDst = len3(L);
    L = norm3(L);
    if (dot3(L, N) > 0.f && dot3(L, normalOnLight) < 0.f) {
      cx->st.shadowRays++;
      f3 att = shadow_attenuation(cx, h->frontHitPoint, L, sc->rayEpsilonT, lightDst - sc->rayEpsilonT);
      if (len3(att) != 0.0f) {
        H = norm3(add3(L, V));
        float lightPdf = lightDst * lightDst / light->area / dot3(normalOnLight, neg3(L));
        float objPdf = disney_pdf(m, N, L, V, H);
        if (g_disney_binary64) objPdf = (float)disney_pdf_d(m, Nd, dnorm(d_of(L)), dnorm(dadd(dnorm(d_of(L)), Vd)));
        if (lightPdf > 0 && objPdf > 0) {
          f3 brdf = disney_eval(m, baseColor, N, L, V, H);
          if (g_disney_binary64) brdf = f_of(disney_eval_d(m, baseColor, Nd, dnorm(d_of(L)), Vd, dnorm(dadd(dnorm(d_of(L)), Vd))));
          f3 c = divs3(mul3(mul3(scl3(brdf, powerHeuristic(lightPdf, objPdf)), ld3(light->emission)), att), fmaxf(0.001f, lightPdf));
          direct = add3(direct, c);
        }
      }
    }
  }

  f3 indirect = mk3(0.f, 0.f, 0.f);
  d3 Ld = dmk(0, 0, 1), Hd = dmk(0, 0, 1);
  if (g_disney_binary64) { disney_sample_d(&p->randSeed, m, Nd, Vd, &Ld, &Hd); L = f_of(Ld); H = f_of(Hd); }
  else disney_sample(&p->randSeed, m, N, V, &L, &H);
  if (dot3(N, L) > 0.0f && dot3(N, V) > 0.0f) {
    Payload c = fork_payload(p);
    cx->st.bounceRays++;
    trace_radiance(cx, h->frontHitPoint, L, sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &c);
    float pdf = g_disney_binary64 ? (float)disney_pdf_d(m, Nd, Ld, Hd) : disney_pdf(m, N, L, V, H);
    if (pdf > 0) {
      f3 brdf = g_disney_binary64 ? mk3(0.f, 0.f, 0.f) : disney_eval(m, baseColor, N, L, V, H);
      if (g_disney_binary64) {      /* brdf / pdf in binary64 as well */
        const double pd = disney_pdf_d(m, Nd, Ld, Hd);
        const d3 bd = disney_eval_d(m, baseColor, Nd, Ld, Vd, Hd);
        indirect = mk3((float)(bd.x / pd * c.color.x), (float)(bd.y / pd * c.color.y), (float)(bd.z / pd * c.color.z));
      } else
      indirect = divs3(mul3(brdf, c.color), pdf);
    }
  }
  if (g_indirect_scale_pct != 100) indirect = scl3(indirect, (float)g_indirect_scale_pct * 0.01f);
  if (g_indirect_depth1_off && p->depth == 1) indirect = mk3(0.f, 0.f, 0.f);
  p->color = add3(add3(indirect, direct), ld3(m->emission));
}

/* rtTrace for ray type 0: nearest hit -> closest-hit program; none -> miss.cu:10-12 */
static void trace_radiance(Ctx* cx, f3 o, f3 d, float tmin, float tmax, Payload* pld) {
  Hit h;
  if (pld->depth > cx->maxDepth) cx->maxDepth = pld->depth;
  if (!find_closest(cx, o, d, tmin, tmax, &h)) {
    cx->st.misses++;
    pld->color = mul3(pld->color, ld3(cx->sc->bgColor));
    return;
  }
  cx->st.closestHits++;
  const OrcMaterial* m = &cx->sc->materials[h.mat];
  switch (m->kind) {
    case ORC_LAMBERTIAN: prog_lambertian(cx, m, o, d, &h, pld); break;
    case ORC_METAL:      prog_metal(cx, m, o, d, &h, pld); break;
    case ORC_GLASS:      prog_glass(cx, m, d, &h, pld); break;
    case ORC_DISNEY:     prog_disney(cx, m, d, &h, pld); break;
    case ORC_LIGHT:      pld->color = ld3(m->emission); break;   /* Material.cu:238-240 */
    default: break;
  }
}

void orc_trace_one(const OrcScene* sc, const float org[3], const float dir[3], int32_t seed, float outColor[3]) {
  Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc;
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
  cx.bvh = bvh;
  Payload p; p.depth = 1; p.randSeed = seed; p.color = mk3(1.f, 1.f, 1.f);
  trace_radiance(&cx, ld3(org), ld3(dir), sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &p);
  st3(outColor, p.color);
  bvh_free(bvh);
}

/* Camera.cu:21-42 for one pixel and one launch seed */
static f3 camera_sample(Ctx* cx, int32_t x, int32_t y, int32_t launchSeed) {
  const OrcScene* sc = cx->sc;
  const OrcCam* cam = &sc->cam;
  Payload pld;
  pld.depth = 1;
  pld.randSeed = (int32_t)orc_tea16((uint32_t)y * (uint32_t)sc->width + (uint32_t)x, (uint32_t)launchSeed);
  pld.color = mk3(1.f, 1.f, 1.f);
  f3 randInLens = scl3(rand_in_unit_disk(&pld.randSeed), cam->lensRadius);
  f3 offs = add3(scl3(ld3(cam->u), randInLens.x), scl3(ld3(cam->v), randInLens.y));
  float r1 = orc_rand(&pld.randSeed); float r2 = orc_rand(&pld.randSeed);
  if (g_draw_order & 4) { float t_ = r1; r1 = r2; r2 = t_; }
  float xyx = ((float)x + r1 - 0.5f) / (float)sc->width;
  float xyy = ((float)y + r2 - 0.5f) / (float)sc->height;
  f3 org = add3(ld3(cam->origin), offs);
  f3 dir = norm3(sub3(sub3(add3(add3(ld3(cam->scrLowerLeftCorner), scl3(ld3(cam->horizontal), xyx)),
                                 scl3(ld3(cam->vertical), xyy)), ld3(cam->origin)), offs));
  cx->st.primaryRays++; cx->st.samples++;
  trace_radiance(cx, org, dir, sc->rayEpsilonT, ORC_RT_DEFAULT_MAX, &pld);
  cx->lastRaw = pld.color;                                  /* analysis: the sample before Camera.cu:39 */
  return mk3(clampf(pld.color.x, 0.f, 1.f), clampf(pld.color.y, 0.f, 1.f), clampf(pld.color.z, 0.f, 1.f));
}

/* MinimalOptiX.cpp:562-585; gravity 4000, attenuation 0.9 (MinimalOptiX.h:23-24) */
void orc_move_sphere(float c[3], float radius, float v[3], float time) {
  const float gravity = 4000.f, attenuationCoef = 0.9f;
  for (;;) {
    float distance = v[1] * time + time * time * gravity / 2.0f;
    if (distance < c[1] - radius + 0.5f) {
      c[0] += v[0] * time; c[2] += v[2] * time; c[1] -= distance; v[1] += gravity * time;
      return;
    }
    float vend = sqrtf(fmaxf(0.0f, v[1] * v[1] + (2.0f * gravity * (c[1] - radius + 0.5f))));   /* D7: NaN guard, see DESIGN.md */
    float t = (vend - v[1]) / gravity;
    if (t < 1e-6) { v[1] = 0.f; c[1] = -0.5f + radius; return; }
    c[0] += v[0] * t; c[2] += v[2] * t; c[1] = -0.5f + radius;
    v[0] *= attenuationCoef; v[1] *= attenuationCoef; v[1] = -vend * attenuationCoef;
    time = time - t;
  }
}

/* ANALYSIS ONLY (DESIGN.md "coffee.png pin"): the reference's context has a 9608-byte OptiX stack (MinimalOptiX.cpp:134) and an
 * exception program that adds badColor = (1,1,1) to the pixel INSTEAD of the sample (Exception.cu:10-12, MinimalOptiX.cpp:149-151)
 * when the recursion overflows it.  At which nesting depth that happens is an OptiX 5.1 internal; this entry returns, per pixel,
 * the sum of the clamped sample colours and the number of samples by the deepest radiance rtTrace of the sample
 * (bucket k = depth k, k = 1..nBuckets-1; the last bucket collects everything deeper), so that
 *   image(D) = (sum_{k<D} colour[k] + sum_{k>=D} count[k] * badColor) / spp
 * can be formed for every candidate overflow depth D from one render.  colourSum: [H][W][nBuckets][3], count: [H][W][nBuckets]
 * (only rows/columns of the region are written). */
int orc_render_by_depth(const OrcScene* sc, const int32_t* seeds, int nSeeds, int x0, int y0, int x1, int y1,
                        int nBuckets, float* colourSum, float* count) {
  if (!sc || !colourSum || !count || nBuckets < 2) return -1;
  if (x0 < 0 || y0 < 0 || x1 > sc->width || y1 > sc->height || x0 > x1 || y0 > y1) return -2;
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
  const int rows = y1 - y0;
#pragma omp parallel
  {
    Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc; cx.bvh = bvh;
#pragma omp for schedule(dynamic, 1)
    for (int r = 0; r < rows; r++) {
      int y = y0 + r;
      for (int x = x0; x < x1; x++) {
        const size_t px = (size_t)y * (size_t)sc->width + (size_t)x;
        for (int s = 0; s < nSeeds; s++) {
          cx.maxDepth = 0;
          f3 c = camera_sample(&cx, x, y, seeds[s]);
          int k = cx.maxDepth < nBuckets - 1 ? cx.maxDepth : nBuckets - 1;
          float* cs = colourSum + 3 * (px * (size_t)nBuckets + (size_t)k);
          cs[0] += c.x; cs[1] += c.y; cs[2] += c.z;
          count[px * (size_t)nBuckets + (size_t)k] += 1.f;
        }
      }
    }
  }
  bvh_free(bvh);
  return 0;
}

/* ANALYSIS ONLY: what the per-sample clamp (Camera.cu:39) does in a region.  Per pixel and channel: the sum of the samples
 * before the clamp (each capped at `cap` so that one firefly cannot own the mean), the number of samples above 1, and the
 * sum of the clamped samples (= what orc_render accumulates).  Arrays are [H][W][3]. */
int orc_render_clamp_stats(const OrcScene* sc, const int32_t* seeds, int nSeeds, int x0, int y0, int x1, int y1, float cap,
                           float* rawSum, float* nClamped, float* clampedSum) {
  if (!sc || !rawSum || !nClamped || !clampedSum) return -1;
  if (x0 < 0 || y0 < 0 || x1 > sc->width || y1 > sc->height || x0 > x1 || y0 > y1) return -2;
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
  const int rows = y1 - y0;
#pragma omp parallel
  {
    Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc; cx.bvh = bvh;
#pragma omp for schedule(dynamic, 1)
    for (int r = 0; r < rows; r++) {
      int y = y0 + r;
      for (int x = x0; x < x1; x++) {
        const size_t px = 3 * ((size_t)y * (size_t)sc->width + (size_t)x);
        for (int s = 0; s < nSeeds; s++) {
          f3 c = camera_sample(&cx, x, y, seeds[s]);
          const float raw[3] = { cx.lastRaw.x, cx.lastRaw.y, cx.lastRaw.z }, cl[3] = { c.x, c.y, c.z };
          for (int k = 0; k < 3; k++) {
            rawSum[px + k] += raw[k] < cap ? raw[k] : cap;      /* NaN compares false: counted as cap */
            nClamped[px + k] += raw[k] > 1.f ? 1.f : 0.f;
            clampedSum[px + k] += cl[k];
          }
        }
      }
    }
  }
  bvh_free(bvh);
  return 0;
}

int orc_num_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

int orc_render(const OrcScene* sc, const int32_t* seeds, int nSeeds, float* accum,
               int x0, int y0, int x1, int y1, int nThreads, OrcStats* stats) {
  if (!sc || !accum || (!seeds && nSeeds > 0)) return -1;
  if (x0 < 0 || y0 < 0 || x1 > sc->width || y1 > sc->height || x0 > x1 || y0 > y1) return -2;
  for (int32_t f = 0; f < 3 * sc->nFaces; f++) if (sc->vIdx[f] < 0 || sc->vIdx[f] >= sc->nVerts) return -3;
  TriBVH* bvh = (sc->nFaces > 0 && !sc->bruteForceTris) ? bvh_build(sc) : NULL;
  OrcStats total; memset(&total, 0, sizeof(total));
#ifdef _OPENMP
  if (nThreads > 0) omp_set_num_threads(nThreads);
#else
  (void)nThreads;
#endif
  const int rows = y1 - y0;
#pragma omp parallel
  {
    Ctx cx; memset(&cx, 0, sizeof(cx)); cx.sc = sc; cx.bvh = bvh;
#pragma omp for schedule(dynamic, 1)
    for (int r = 0; r < rows; r++) {
      int y = y0 + r;
      for (int x = x0; x < x1; x++) {
        float* px = accum + 3 * ((size_t)y * (size_t)sc->width + (size_t)x);
        for (int s = 0; s < nSeeds; s++) {      /* one launch per seed, in order (MinimalOptiX.cpp:544-546) */
          f3 c = camera_sample(&cx, x, y, seeds[s]);
          px[0] += c.x; px[1] += c.y; px[2] += c.z;   /* Camera.cu:41 */
        }
      }
    }
#pragma omp critical
    {
      total.primaryRays += cx.st.primaryRays; total.bounceRays += cx.st.bounceRays; total.shadowRays += cx.st.shadowRays;
      total.samples += cx.st.samples; total.closestHits += cx.st.closestHits; total.misses += cx.st.misses;
      total.depthCapped += cx.st.depthCapped;
    }
  }
  bvh_free(bvh);
  if (stats) *stats = total;
  return 0;
}
