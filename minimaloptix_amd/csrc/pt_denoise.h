// pt_denoise.h -- per-pixel code of the edge-aware a-trous denoiser (include/moptix.h "denoiser", DESIGN.md "Denoiser").
//
// The edge-avoiding a-trous wavelet transform (Dammertz et al. 2010) with SVGF's luminance-variance edge stop (Schied et al. 2017),
// spatial part only, guided by the first-hit AOVs.  Every pass is a function of one pixel over the previous pass's buffers, so the
// kernels (denoisekernel.hip) and their CPU mirror (tests/denoisesim) run exactly these operations in the same order and agree bit for
// bit.  The arithmetic follows the contract of pt_math.h (AC1-AC5, -ffp-contract=off): every operation not written as fma_ / dot is
// one IEEE binary32 operation, and the one transcendental, exp, is exp_ac below -- no libm call.
//
// Buffers, per pixel p = y * width + x (row 0 = bottom, the accumulation buffer's layout):
//   col   {I.rgb, v}   the filtered signal (demodulated beauty) and its variance; ping-pong between passes
//   guide {N.xyz, Z}   normal and depth; Z = kDnBackground marks a background pixel (hits == 0), which is never a tap
//   side  {a.rgb, g}   the remodulation factor max(A, 1e-3) (1 without demodulation) and the depth gradient; read by p alone
// Passes: dn_decode (inputs -> col, guide, side), dn_prepass (3x3 variance and depth gradient), `iterations` x dn_iterate (5x5
// taps at step 2^i), dn_final (remodulate).  Background pixels carry C through every pass unchanged.
#pragma once
#include "pt_math.h"

namespace pt {

constexpr float kDnBackground = -__builtin_inff();     // guide.w of a background pixel
constexpr float kDnAlbedoFloor = 1e-3f;
constexpr float kDnEps = 1e-4f;

// e^x as ONE specified binary32 algorithm, as AC5 specifies sin / cos.  x < -87 (and NaN) -> 0: e^-87 = 1.6e-38 is the last value kept, just
// above FLT_MIN, so no subnormal is ever formed; x > 88 -> +inf.  Otherwise k = floor(x * log2(e) + 1/2), Cody-Waite reduction
// r = x - k ln2 in two fma steps (ln2 = 0.693359375 - 2.12194440e-4), e^r = 1 + r + r^2 P(r) with the degree-5 polynomial of the
// classic single-precision kernel (|r| <= ln2 / 2), and 2^k built from its exponent bits.  exp_ac(0) = 1 exactly; relative error
// below 2^-21 on [-87, 0] (tests/test_denoise_cpu.py).
PT_HD float exp_ac(float x) {
  if (!(x >= -87.0f)) return 0.0f;
  if (x > 88.0f) return __builtin_inff();
  const float kf = __builtin_floorf(fma_(x, 1.44269504088896341f, 0.5f));
  float r = fma_(kf, -0.693359375f, x);
  r = fma_(kf, 2.12194440e-4f, r);
  const float z = r * r;
  float p = fma_(1.9875691500e-4f, r, 1.3981999507e-3f);
  p = fma_(p, r, 8.3334519073e-3f);
  p = fma_(p, r, 4.1665795894e-2f);
  p = fma_(p, r, 1.6666665459e-1f);
  p = fma_(p, r, 5.0000001201e-1f);
  const float y = fma_(p, z, r) + 1.0f;
  return y * i2f(((int32_t)kf + 127) << 23);
}

// x^n for n >= 1 by binary exponentiation, least significant bit first:
//   r = 1, b = x; loop { if (n & 1) r = r * b; n >>= 1; if (n == 0) stop; b = b * b; }
PT_HD float pow_int_ac(float x, int n) {
  float r = 1.0f, b = x;
  for (;;) {
    if (n & 1) r = r * b;
    n >>= 1;
    if (n == 0) return r;
    b = b * b;
  }
}

// l(I) = (0.2126 r + 0.7152 g) + 0.0722 b
PT_HD float dn_luminance(v3 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

PT_HD bool dn_geometry(const v4& guide) { return guide.w != kDnBackground; }

// What the per-pixel passes read besides the buffers.
struct DenoiseConsts {
  int width, height;
  int normalPower;              // 1..256
  float sigmaLuminance, sigmaDepth;
};

// The argument check of moptix_denoise and moptix_denoise_temporal: null when nAccumulation and the moptix_denoise_params members are in
// range, else what is wrong with them.
PT_HD const char* dn_bad_params(float nAccumulation, int iterations, int normalPower, int demodulate, float sigmaLuminance, float sigmaDepth) {
  if (!(nAccumulation > 0.0f) || !__builtin_isfinite(nAccumulation)) return "nAccumulation must be > 0";
  if (iterations < 0 || iterations > 8) return "iterations in [0,8]";
  if (normalPower < 1 || normalPower > 256) return "normalPower in [1,256]";
  if (demodulate != 0 && demodulate != 1) return "demodulate is 0 or 1";
  if (!(sigmaLuminance >= 0.0f) || !__builtin_isfinite(sigmaLuminance) || !(sigmaDepth >= 0.0f) || !__builtin_isfinite(sigmaDepth))
    return "sigmas must be finite and >= 0";
  return nullptr;
}

// Pass 1, pixel p: C = accum / nAcc, and for a geometry pixel (hits > 0) A = albedo / S, N = normalize(normal / S) (0 where that is
// 0), Z = depth / hits -- each division one IEEE operation per component, normalize as AC3.  demodulate: I = C / max(A, 1e-3) per
// channel, else I = C.  A background pixel stores I = C, guide (0, 0, 0, kDnBackground) and a = 1.
PT_HD void dn_decode(const float* accum, const float* albedo, const float* normal, const float* depth, const float* hits,
                     float nAccumulation, float nSamples, int demodulate, int p, v4& col, v4& guide, v4& side) {
  const size_t p3 = 3 * (size_t)p;
  const v3 c = mk3(accum[p3] / nAccumulation, accum[p3 + 1] / nAccumulation, accum[p3 + 2] / nAccumulation);
  const float h = hits[p];
  if (!(h > 0.0f)) {
    col = mk4(c.x, c.y, c.z, 0.0f); guide = mk4(0.0f, 0.0f, 0.0f, kDnBackground); side = mk4(1.0f, 1.0f, 1.0f, 0.0f);
    return;
  }
  v3 a = mk3(1.0f, 1.0f, 1.0f), i = c;
  if (demodulate) {
    a = mk3(fmaxf_(albedo[p3] / nSamples, kDnAlbedoFloor), fmaxf_(albedo[p3 + 1] / nSamples, kDnAlbedoFloor),
            fmaxf_(albedo[p3 + 2] / nSamples, kDnAlbedoFloor));
    i = mk3(c.x / a.x, c.y / a.y, c.z / a.z);
  }
  const v3 n = mk3(normal[p3] / nSamples, normal[p3 + 1] / nSamples, normal[p3 + 2] / nSamples);
  const v3 nn = dot(n, n) != 0.0f ? normalize(n) : mk3(0.0f, 0.0f, 0.0f);
  col = mk4(i.x, i.y, i.z, 0.0f); guide = mk4(nn.x, nn.y, nn.z, depth[p] / h); side = mk4(a.x, a.y, a.z, 0.0f);
}

// |Z+ - Z-| / 2 with both neighbours of an axis, the one-sided |Z_n - Z_p| with one, 0 with none
PT_HD float dn_axis_gradient(bool lo, bool hi, float zl, float z, float zh) {
  return (lo && hi) ? __builtin_fabsf(zh - zl) * 0.5f : lo ? __builtin_fabsf(z - zl) : hi ? __builtin_fabsf(zh - z) : 0.0f;
}

// Pass 2, geometry pixel (x, y): the variance v of l(I) over the geometry pixels of the 3x3 window (row-major sums s1 = sum l,
// s2 = sum l^2, n; v = max(0, s2 / n - (s1 / n)^2)) and the depth gradient g = max(gx, gy), where per axis
// g = |Z+ - Z-| / 2 with both neighbours geometry, |Z_n - Z_p| with one, 0 with none.  Returns v; g goes to side.w.
PT_HD float dn_prepass(const DenoiseConsts& k, const v4* col, const v4* guide, int x, int y, float& g) {
  float s1 = 0.0f, s2 = 0.0f, n = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= k.height) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= k.width) continue;
      const int q = qy * k.width + qx;
      if (!dn_geometry(guide[q])) continue;
      const float l = dn_luminance(xyz(col[q]));
      s1 = s1 + l; s2 = s2 + l * l; n = n + 1.0f;
    }
  }
  const float m1 = s1 / n, m2 = s2 / n;
  const float v = fmaxf_(m2 - m1 * m1, 0.0f);
  const int p = y * k.width + x;
  const float z = guide[p].w;
  const bool west = x > 0 && dn_geometry(guide[p - 1]), east = x + 1 < k.width && dn_geometry(guide[p + 1]);
  const bool south = y > 0 && dn_geometry(guide[p - k.width]), north = y + 1 < k.height && dn_geometry(guide[p + k.width]);
  const float gx = dn_axis_gradient(west, east, west ? guide[p - 1].w : 0.0f, z, east ? guide[p + 1].w : 0.0f);
  const float gy = dn_axis_gradient(south, north, south ? guide[p - k.width].w : 0.0f, z, north ? guide[p + k.width].w : 0.0f);
  g = fmaxf_(gx, gy);
  return v;
}

// B3 spline weights h(-2..2) and the 3x3 blur's (1/4, 1/2, 1/4); products of two of them are exact in binary32
PT_HD float dn_h5(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }
PT_HD float dn_h3(int d) { return d == 0 ? 0.5f : 0.25f; }

// Pass 3 (one iteration at step = 2^i), geometry pixel (x, y) with depth gradient g:
//   G3(v)_p = sum h3(dx) h3(dy) v_q / sum h3(dx) h3(dy) over the geometry pixels q of the 3x3 window (row-major)
//   den_l = sigmaLuminance * sqrt(G3(v)_p) + 1e-4
//   taps q = p + step (dx, dy), dy outer, dx inner, -2..2; outside the frame or background: skipped
//     centre (dx = dy = 0): w = 9/64
//     else: w_n = pow_int_ac(max(0, dot(N_p, N_q)), normalPower)
//           w_z = exp_ac(-(|Z_p - Z_q| / ((sigmaDepth * (step (|dx| + |dy|))) * g + 1e-4)))
//           w_l = exp_ac(-(|l_p - l_q| / den_l))
//           w = (((h(dx) h(dy)) * w_n) * w_z) * w_l
//     sw += w; sI += w * I_q (per channel); sv += (w * w) * v_q
//   I' = sI / sw (per channel), v' = sv / (sw * sw)
PT_HD v4 dn_iterate(const DenoiseConsts& k, const v4* col, const v4* guide, int x, int y, int step, float g) {
  const int p = y * k.width + x;
  const v4 cp = col[p], gp = guide[p];
  float sv3 = 0.0f, sk3 = 0.0f;
  for (int dy = -1; dy <= 1; dy++) {
    const int qy = y + dy;
    if (qy < 0 || qy >= k.height) continue;
    for (int dx = -1; dx <= 1; dx++) {
      const int qx = x + dx;
      if (qx < 0 || qx >= k.width) continue;
      const int q = qy * k.width + qx;
      if (!dn_geometry(guide[q])) continue;
      const float w = dn_h3(dx) * dn_h3(dy);
      sv3 = sv3 + w * col[q].w; sk3 = sk3 + w;
    }
  }
  const float denL = k.sigmaLuminance * __builtin_sqrtf(sv3 / sk3) + kDnEps;
  const v3 np = xyz(gp);
  const float lp = dn_luminance(xyz(cp));
  float sw = 0.0f, sv = 0.0f;
  v3 si = mk3(0.0f, 0.0f, 0.0f);
  for (int dy = -2; dy <= 2; dy++) {
    const int qy = y + step * dy;
    if (qy < 0 || qy >= k.height) continue;
    for (int dx = -2; dx <= 2; dx++) {
      const int qx = x + step * dx;
      if (qx < 0 || qx >= k.width) continue;
      const int q = qy * k.width + qx;
      const v4 gq = guide[q];
      if (!dn_geometry(gq)) continue;
      const v4 cq = col[q];
      float w;
      if (dx == 0 && dy == 0) {
        w = 0.140625f;
      } else {
        const float wn = pow_int_ac(fmaxf_(dot(np, xyz(gq)), 0.0f), k.normalPower);
        const int dist = step * (__builtin_abs(dx) + __builtin_abs(dy));
        const float wz = exp_ac(-(__builtin_fabsf(gp.w - gq.w) / ((k.sigmaDepth * (float)dist) * g + kDnEps)));
        const float wl = exp_ac(-(__builtin_fabsf(lp - dn_luminance(xyz(cq))) / denL));
        w = (((dn_h5(dx) * dn_h5(dy)) * wn) * wz) * wl;
      }
      sw = sw + w;
      si = mk3(si.x + w * cq.x, si.y + w * cq.y, si.z + w * cq.z);
      sv = sv + (w * w) * cq.w;
    }
  }
  return mk4(si.x / sw, si.y / sw, si.z / sw, sv / (sw * sw));
}

// Pass 4, pixel p: geometry -> I' * a per channel; background -> the C it carried.  Writes float3 at out[3p].
PT_HD void dn_final(const v4& col, const v4& guide, const v4& side, float* out, int p) {
  const size_t p3 = 3 * (size_t)p;
  if (dn_geometry(guide)) { out[p3] = col.x * side.x; out[p3 + 1] = col.y * side.y; out[p3 + 2] = col.z * side.z; }
  else                    { out[p3] = col.x; out[p3 + 1] = col.y; out[p3 + 2] = col.z; }
}

}  // namespace pt
