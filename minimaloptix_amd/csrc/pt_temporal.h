// pt_temporal.h -- per-pixel code of the denoiser's temporal stage (include/moptix.h "denoiser: temporal accumulation", DESIGN.md
// "Denoiser").
//
// SVGF's temporal half (Schied et al. 2017) in front of the a-trous iterations of pt_denoise.h: the previous call's pre-filter
// accumulation is reprojected through the first-hit geometry (depth, normal, material id, the two cameras, the spheres' motion),
// blended with this frame's demodulated beauty, and the temporal luminance moments replace the 3x3 spatial variance guess where a pixel
// has enough history.  As in pt_denoise.h every pass is a function of one pixel over buffers of the previous pass or call, so the
// kernels (temporalkernel.hip) and their CPU mirror (tests/temporalsim) run exactly these operations in this order and agree bit for
// bit; the arithmetic follows the contract of pt_math.h (AC1-AC5, -ffp-contract=off, no libm transcendental).
// With the option "temporal_face_motion" a pixel on a moved triangle is reprojected through the triangle's own affine motion
// (tp_face_record per face, facemotionkernel.hip; tp_face_motion per pixel; the mirror of the whole call is tests/facemotionsim).
//
// History, per pixel, three 16-byte records (one vector load per tap each):
//   col   {I_acc.rgb, h}        the pre-filter accumulation and the history length (an integer kept as binary32)
//   guide {N.xyz, Z}            the frame's normal and depth as dn_decode wrote them (Z = kDnBackground: never a tap); the same buffer
//                               guides the a-trous passes of the call that wrote it
//   mom   {m1, m2, matId, 0}    luminance moments; the material id rides in the spare third component as its bits (i2f), so the
//                               material test costs no load of its own
#pragma once
#include "pt_denoise.h"

namespace pt {

constexpr float kTpMinWeight = 1e-2f;         // total weight of the valid taps below which a pixel counts as disoccluded
constexpr float kTpSpatialVariance = -1.0f;   // col.w after tp_reproject where the prepass takes the 3x3 spatial estimate

struct TpCamera { v3 origin, horizontal, vertical, lowerLeft; };

// What tp_reproject reads besides the buffers; all wave-uniform (kernel arguments).
struct TemporalConsts {
  int width, height;
  int haveHistory;              // 0: first frame after a drop, every pixel h = 1
  int sameCamera;               // the previous camera is this one bit for bit
  int nSpheres;                 // entries of the motion buffer (0 without history)
  int maxHistory, varianceFrames;
  float alpha, alphaMoments, depthTolerance, normalThreshold;
  TpCamera cam;                 // this frame's
  v3 prevOrigin;                // o'
  v3 bc, ca, ab;                // cross(b, c), cross(c, a), cross(a, b) of a = LL' - o', b = H', c = V'
  float det;                    // dot(a, bc)
};

// The check of moptix_temporal_params: null when its members are in range, else what is wrong with them.
PT_HD const char* tp_bad_params(float alpha, float alphaMoments, float depthTolerance, float normalThreshold, int maxHistory, int varianceFrames) {
  if (!(alpha >= 0.0f && alpha <= 1.0f) || !(alphaMoments >= 0.0f && alphaMoments <= 1.0f)) return "alpha and alphaMoments in [0,1]";      // NaN fails
  if (!__builtin_isfinite(depthTolerance) || !(depthTolerance >= 0.0f)) return "depthTolerance must be finite and >= 0";
  if (!(normalThreshold >= -1.0f && normalThreshold <= 1.0f)) return "normalThreshold in [-1,1]";
  if (maxHistory < 1 || maxHistory > 65536) return "maxHistory in [1,65536]";
  if (varianceFrames < 1 || varianceFrames > 65536) return "varianceFrames in [1,65536]";
  return nullptr;
}

// The 3x3 solve's constants from the previous camera.
PT_HD void tp_solve_consts(const TpCamera& prev, TemporalConsts& k) {
  const v3 a = prev.lowerLeft - prev.origin, b = prev.horizontal, c = prev.vertical;
  k.prevOrigin = prev.origin;
  k.bc = cross(b, c); k.ca = cross(c, a); k.ab = cross(a, b);
  k.det = dot(a, k.bc);
}

PT_HD bool tp_same_camera(const TpCamera& p, const TpCamera& q) {
  const float* a = &p.origin.x; const float* b = &q.origin.x;
  for (int i = 0; i < 12; i++) if (f2i(a[i]) != f2i(b[i])) return false;
  return true;
}

// Is the history of the previous call usable for this one?  (step 8 of the contract: frame size, sphere count, demodulation)
PT_HD bool tp_history_kept(bool have, int prevW, int prevH, int prevSpheres, int prevDemodulate, int w, int h, int nSpheres, int demodulate) {
  return have && prevW == w && prevH == h && prevSpheres == nSpheres && prevDemodulate == demodulate;
}

// ---- per-face motion (option "temporal_face_motion") ----
// What tp_reproject_faces reads besides tp_reproject's arguments; wave-uniform.  nTracked == 0: off.
struct TpFaces {
  const float* pos;             // the faces' positions now, 9 floats per face (p0 p1 p2), upload order
  const v4* rec;                // three records per face: {d0, moved flag bits}, {d1, 0}, {d2, 0}; d_i = p_i(now) - p_i(prev)
  int first;                    // primId of face 0: nSpheres + nQuads
  int nTracked;                 // faces with a record
};

constexpr int kTpFaceMoved = 1;               // rec[3 f].w as bits: a displacement component of face f is not zero

// One face's record from its positions now and at the snapshot; true = moved.
PT_HD bool tp_face_record(const float* now, const float* prev, v4* rec) {
  float d[9];
  bool moved = false;
  for (int i = 0; i < 9; i++) { d[i] = now[i] - prev[i]; moved = moved || d[i] != 0.0f; }
  rec[0] = mk4(d[0], d[1], d[2], i2f(moved ? kTpFaceMoved : 0));
  rec[1] = mk4(d[3], d[4], d[5], 0.0f);
  rec[2] = mk4(d[6], d[7], d[8], 0.0f);
  return moved;
}

// The motion of world point P on a moved face: the triangle's affine motion at the projection of P onto its plane.
//   e1 = p1 - p0, e2 = p2 - p0, n = cross(e1, e2), nn = dot(n, n), w = P - p0
//   nn > 0: bu = dot(cross(w, e2), n) / nn, bv = dot(cross(e1, w), n) / nn, each clamped to [-1, 2]; else bu = bv = 0
//   mo = (d0 + bu * (d1 - d0)) + bv * (d2 - d0) per component
PT_HD v3 tp_face_motion(const float* p, const v3& d0, const v3& d1, const v3& d2, const v3& P) {
  const v3 p0 = mk3(p[0], p[1], p[2]);
  const v3 e1 = mk3(p[3], p[4], p[5]) - p0, e2 = mk3(p[6], p[7], p[8]) - p0;
  const v3 n = cross(e1, e2);
  const float nn = dot(n, n);
  const v3 w = P - p0;
  float bu = 0.0f, bv = 0.0f;
  if (nn > 0.0f) {
    bu = fminf_(fmaxf_(dot(cross(w, e2), n) / nn, -1.0f), 2.0f);
    bv = fminf_(fmaxf_(dot(cross(e1, w), n) / nn, -1.0f), 2.0f);
  }
  return mk3((d0.x + bu * (d1.x - d0.x)) + bv * (d2.x - d0.x), (d0.y + bu * (d1.y - d0.y)) + bv * (d2.y - d0.y),
             (d0.z + bu * (d1.z - d0.z)) + bv * (d2.z - d0.z));
}

// Step 1: the world point of pixel (x, y) at depth Z.
PT_HD v3 tp_world_point(const TemporalConsts& k, int x, int y, float Z) {
  const float u = ((float)x + 0.5f) / (float)k.width, v = ((float)y + 0.5f) / (float)k.height;
  const v3 t = mk3(((k.cam.lowerLeft.x + u * k.cam.horizontal.x) + v * k.cam.vertical.x) - k.cam.origin.x,
                   ((k.cam.lowerLeft.y + u * k.cam.horizontal.y) + v * k.cam.vertical.y) - k.cam.origin.y,
                   ((k.cam.lowerLeft.z + u * k.cam.horizontal.z) + v * k.cam.vertical.z) - k.cam.origin.z);
  return ray_at(k.cam.origin, normalize(t), Z);
}

struct TpResult {
  v4 col;             // {I_acc, v or kTpSpatialVariance}: the a-trous input
  v4 hist;            // {I_acc, h}
  v4 mom;             // {m1, m2, matId bits, 0}
  float mvx, mvy;     // motion vector (x - fx, y - fy); 0 without history
  bool geometry, history;
  bool movedFace;     // tp_reproject_faces: a geometry pixel with history to look for whose face has moved
};

// Steps 1-6 for pixel (x, y) whose decoded signal, guide and ids are (col.xyz = I, guide = {N, Z}).  motion[i] = centre_now -
// centre_prev of sphere i (k.nSpheres entries).  Operation order:
//   u = (x + 0.5) / W, v = (y + 0.5) / H                                 (int -> float conversions exact)
//   t = ((LL + u * Hz) + v * V) - o per component; d = normalize(t) (AC3); P = fma(Z, d, o) (AC7)
//   P' = P - motion[primId] per component when 0 <= primId < nSpheres
//   kFaces: f = primId - faces.first; when 0 <= f < faces.nTracked and rec[3 f].w says moved, P' = P - tp_face_motion(...)
//   r = P' - o'; sn = dot(r, bc); s = sn / det; no history unless det != 0 and s > 0
//   fx = (dot(r, ca) / sn) * W - 0.5, fy = (dot(r, ab) / sn) * H - 0.5; Z' = length(r)
//   (the same camera bit for bit and a zero motion: fx = x, fy = y, Z' = Z exactly -- a static pixel maps onto itself)
//   no history unless -1 < fx < W and -1 < fy < H; x0 = floor(fx), tx = fx - x0 (y alike)
//   taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1) in this order, weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty;
//     a tap counts iff its weight > 0, it is inside the frame, geometry in the previous frame, of the same material,
//     dot(N_p, N_q) >= normalThreshold and |Z_q - Z'| <= depthTolerance * Z'
//     sw += w; sI += w * I_q (per channel); s1 += w * m1_q; s2 += w * m2_q; hmin = min(hmin, h_q)
//   history iff a tap counted and sw >= 1e-2: I_prev = sI / sw, m1_prev = s1 / sw, m2_prev = s2 / sw (one division each)
//   h = min(hmin + 1, maxHistory); a = max(1 / h, alpha); I_acc = I_prev + a * (I - I_prev); moments alike with alphaMoments on
//   l = l(I), l * l; without history h = 1, I_acc = I, m1 = l, m2 = l * l
//   v = h >= varianceFrames ? max(0, m2 - m1 * m1) : kTpSpatialVariance
template <bool kFaces>
PT_HD TpResult tp_reproject_t(const TemporalConsts& k, const v4* histCol, const v4* histGuide, const v4* histMom, const v4* motion,
                              const TpFaces& faces, int x, int y, const v4& col, const v4& guide, int primId, int matId) {
  TpResult o;
  o.mvx = 0.0f; o.mvy = 0.0f; o.history = false; o.movedFace = false;
  o.geometry = dn_geometry(guide);
  const v3 I = xyz(col);
  if (!o.geometry) {
    o.col = mk4(I.x, I.y, I.z, 0.0f); o.hist = mk4(I.x, I.y, I.z, 1.0f); o.mom = mk4(0.0f, 0.0f, i2f(matId), 0.0f);
    return o;
  }
  const float l = dn_luminance(I);
  v3 sI = mk3(0.0f, 0.0f, 0.0f);
  float sw = 0.0f, s1 = 0.0f, s2 = 0.0f, hmin = 0.0f;
  bool any = false;
  float fx = 0.0f, fy = 0.0f;
  if (k.haveHistory) {
    const float Z = guide.w;
    v3 mo = mk3(0.0f, 0.0f, 0.0f);
    if (primId >= 0 && primId < k.nSpheres) mo = xyz(motion[primId]);
    v3 Pf = mk3(0.0f, 0.0f, 0.0f);                             // the world point, where the face lookup already needed it
    if constexpr (kFaces) {
      const int f = primId - faces.first;
      if (f >= 0 && f < faces.nTracked) {
        const v4 r0 = faces.rec[3 * (size_t)f];
        if (f2i(r0.w) != 0) {
          o.movedFace = true;
          Pf = tp_world_point(k, x, y, Z);
          mo = tp_face_motion(faces.pos + 9 * (size_t)f, xyz(r0), xyz(faces.rec[3 * (size_t)f + 1]), xyz(faces.rec[3 * (size_t)f + 2]), Pf);
        }
      }
    }
    const bool still = k.sameCamera && mo.x == 0.0f && mo.y == 0.0f && mo.z == 0.0f;
    bool ok = true;
    float zp = Z;
    if (still) {
      fx = (float)x; fy = (float)y;
    } else {
      const v3 P = kFaces && o.movedFace ? Pf : tp_world_point(k, x, y, Z);
      const v3 r = (P - mo) - k.prevOrigin;
      const float sn = dot(r, k.bc);
      const float s = sn / k.det;
      ok = k.det != 0.0f && s > 0.0f;
      if (ok) {
        fx = (dot(r, k.ca) / sn) * (float)k.width - 0.5f;
        fy = (dot(r, k.ab) / sn) * (float)k.height - 0.5f;
        zp = length(r);
      }
    }
    ok = ok && fx > -1.0f && fx < (float)k.width && fy > -1.0f && fy < (float)k.height;
    if (ok) {
      const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
      const int x0 = (int)flx, y0 = (int)fly;
      const float tx = fx - flx, ty = fy - fly;
      const float ux = 1.0f - tx, uy = 1.0f - ty;
      const v3 np = xyz(guide);
      const float tol = k.depthTolerance * zp;
      for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= k.height) continue;
        for (int i = 0; i < 2; i++) {
          const int qx = x0 + i;
          if (qx < 0 || qx >= k.width) continue;
          const float w = (i ? tx : ux) * (j ? ty : uy);
          if (!(w > 0.0f)) continue;
          const int q = qy * k.width + qx;
          const v4 gq = histGuide[q];
          if (!dn_geometry(gq)) continue;
          const v4 mq = histMom[q];
          if (f2i(mq.z) != matId) continue;
          if (!(dot(np, xyz(gq)) >= k.normalThreshold)) continue;
          if (!(__builtin_fabsf(gq.w - zp) <= tol)) continue;
          const v4 cq = histCol[q];
          sw = sw + w;
          sI = mk3(sI.x + w * cq.x, sI.y + w * cq.y, sI.z + w * cq.z);
          s1 = s1 + w * mq.x; s2 = s2 + w * mq.y;
          hmin = any ? fminf_(hmin, cq.w) : cq.w;
          any = true;
        }
      }
    }
  }
  float h = 1.0f, m1 = l, m2 = l * l;
  v3 acc = I;
  if (any && sw >= kTpMinWeight) {
    o.history = true;
    o.mvx = (float)x - fx; o.mvy = (float)y - fy;
    h = fminf_(hmin + 1.0f, (float)k.maxHistory);
    const float ih = 1.0f / h;
    const float a = fmaxf_(ih, k.alpha), am = fmaxf_(ih, k.alphaMoments);
    const v3 ip = mk3(sI.x / sw, sI.y / sw, sI.z / sw);
    const float p1 = s1 / sw, p2 = s2 / sw;
    acc = mk3(ip.x + a * (I.x - ip.x), ip.y + a * (I.y - ip.y), ip.z + a * (I.z - ip.z));
    m1 = p1 + am * (l - p1);
    m2 = p2 + am * (l * l - p2);
  }
  const float var = h >= (float)k.varianceFrames ? fmaxf_(m2 - m1 * m1, 0.0f) : kTpSpatialVariance;
  o.col = mk4(acc.x, acc.y, acc.z, var);
  o.hist = mk4(acc.x, acc.y, acc.z, h);
  o.mom = mk4(m1, m2, i2f(matId), 0.0f);
  return o;
}

PT_HD TpResult tp_reproject(const TemporalConsts& k, const v4* histCol, const v4* histGuide, const v4* histMom, const v4* motion,
                            int x, int y, const v4& col, const v4& guide, int primId, int matId) {
  return tp_reproject_t<false>(k, histCol, histGuide, histMom, motion, TpFaces{}, x, y, col, guide, primId, matId);
}

// tp_reproject with the triangle case of step 2; faces.nTracked == 0 gives tp_reproject's bits.
PT_HD TpResult tp_reproject_faces(const TemporalConsts& k, const v4* histCol, const v4* histGuide, const v4* histMom, const v4* motion,
                                  const TpFaces& faces, int x, int y, const v4& col, const v4& guide, int primId, int matId) {
  return tp_reproject_t<true>(k, histCol, histGuide, histMom, motion, faces, x, y, col, guide, primId, matId);
}

// The prepass after tp_reproject, geometry pixel (x, y): the depth gradient as dn_prepass, and its 3x3 spatial variance (taken on
// I_acc) only where the temporal one is not there.
PT_HD float tp_prepass(const DenoiseConsts& k, const v4* col, const v4* guide, int x, int y, float& g) {
  const float spatial = dn_prepass(k, col, guide, x, y, g);
  const float v = col[y * k.width + x].w;
  return v == kTpSpatialVariance ? spatial : v;
}

}  // namespace pt
