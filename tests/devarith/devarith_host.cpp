// devarith_host.cpp -- the mirror side of the arithmetic contract tests: the primitives of devarith_ops.h, from the same headers,
// compiled by the host compiler with the flags of the CPU mirrors (the top Makefile hands its CXXFLAGS down).  Linked into
// libdevarith.so beside the kernels; usable without a GPU (da_host_* touch no HIP entry point).
#include <cstddef>
#include <cstdint>
#include <cstring>

#define DA_OP(name, NIN, NOUT, ...)                                                       \
  static void da_host_fn_##name(const float* in, float* out, long n) {                    \
    _Pragma("omp parallel for schedule(static)")                                          \
    for (long i = 0; i < n; i++) {                                                        \
      float x[NIN], y[NOUT];                                                              \
      for (int k = 0; k < NIN; k++) x[k] = in[(size_t)k * n + i];                         \
      __VA_ARGS__                                                                         \
      for (int k = 0; k < NOUT; k++) out[(size_t)k * n + i] = y[k];                       \
    }                                                                                     \
  }
#include "devarith_ops.h"
#undef DA_OP

namespace {
struct Row { const char* name; int nin, nout; void (*fn)(const float*, float*, long); };
#define DA_OP(name, NIN, NOUT, ...) { #name, NIN, NOUT, da_host_fn_##name },
const Row kRows[] = {
#include "devarith_ops.h"
};
#undef DA_OP
}  // namespace

extern "C" {

int da_host_arity(const char* name, int* nin, int* nout) {
  for (const Row& r : kRows)
    if (!strcmp(r.name, name)) { *nin = r.nin; *nout = r.nout; return 0; }
  return -1;
}

int da_host_run(const char* name, const float* in, float* out, long n) {
  for (const Row& r : kRows)
    if (!strcmp(r.name, name)) { r.fn(in, out, n); return 0; }
  return -1;
}

int da_host_tex2d(const float* texels, int width, int height, const float* uv, float* out, long n) {
  if (width < 1 || height < 1) return -2;
  pt::DevTexture t; t.texels = (const pt::v4*)texels; t.width = width; t.height = height;
  _Pragma("omp parallel for schedule(static)")
  for (long i = 0; i < n; i++) {
    const pt::v4 r = pt::tex2d(t, uv[i], uv[(size_t)n + i]);
    out[i] = r.x; out[(size_t)n + i] = r.y; out[(size_t)2 * n + i] = r.z; out[(size_t)3 * n + i] = r.w;
  }
  return 0;
}

// tools/pow22_hard.py: the positive finite binary32 inputs x in [first, last] (bit patterns) whose pt::pow22 is a finite binary32 and
// whose binary64 pow lies within `ulps` binary64 ulps of a binary32 rounding boundary (a midpoint of two neighbouring binary32 values,
// subnormal ones included).  Writes up to cap bit patterns and their distances; returns how many there are.
long da_host_pow22_scan(uint32_t first, uint32_t last, int ulps, uint32_t* bits, int32_t* dist, long cap) {
  long found = 0;
  _Pragma("omp parallel for schedule(static)")
  for (int64_t b = first; b <= (int64_t)last; b++) {
    const uint32_t ub = (uint32_t)b;
    float x; memcpy(&x, &ub, 4);
    const double p = pow((double)x, (double)2.2f);
    const float f = (float)p;
    if (!(f < __builtin_inff()) || !(p > 0.0)) continue;
    // in units of p's binary64 ulp 2^(E-52), binary32 values are 2^s apart at p: s = 29 in the normal range, more below FLT_MIN (the
    // spacing stays 2^-149); the rounding boundaries are the odd multiples of 2^(s-1)
    uint64_t pb; memcpy(&pb, &p, 8);
    const int E = (int)((pb >> 52) & 0x7ff) - 1023;
    const int s = 29 + (E < -126 ? -126 - E : 0);
    if (s > 62) continue;                                           // p < 2^-159: nowhere near the least boundary 2^-150
    const uint64_t sig = (pb & ((1ull << 52) - 1)) | (1ull << 52);
    int64_t d = (int64_t)(sig & ((1ull << s) - 1)) - (int64_t)(1ull << (s - 1));
    if (d < 0) d = -d;
    if (d <= ulps) {
      long at;
      _Pragma("omp atomic capture")
      at = found++;
      if (at < cap) { bits[at] = ub; dist[at] = (int32_t)d; }
    }
  }
  return found;
}

}  // extern "C"
