// atrous_host.h -- TEST INFRASTRUCTURE.  The host statement of launch_atrous (minimaloptix_amd/csrc/denoisekernel.hip): prepass, iterations
// and final in the order the kernels run them, for the CPU mirrors of both entries (denoisesim, temporalsim).
#pragma once
#include <string.h>

#include <vector>

#include "../../minimaloptix_amd/csrc/pt_temporal.h"

namespace pt {

// colA: the decoded (or reprojected) signal; colB: scratch of the same size.  temporalVariance: tp_prepass instead of dn_prepass.
// Optional outputs: pre, W*H*4 floats, the buffer the first iteration reads (after the prepass; colA with iterations = 0), and out, W*H*3.
inline void atrous_host(const DenoiseConsts& k, std::vector<v4>& colA, std::vector<v4>& colB, const v4* guide, v4* side, int iterations,
                        bool temporalVariance, float* pre, float* out) {
  const int n = k.width * k.height, width = k.width;
  v4* cur = colA.data();
  if (iterations > 0) {
#pragma omp parallel for
    for (int p = 0; p < n; p++) {
      v4 c = colA[p];
      if (dn_geometry(guide[p])) {
        float g;
        c.w = temporalVariance ? tp_prepass(k, colA.data(), guide, p % width, p / width, g) : dn_prepass(k, colA.data(), guide, p % width, p / width, g);
        side[p].w = g;
      }
      colB[p] = c;
    }
    cur = colB.data();
  }
  if (pre) memcpy(pre, cur, sizeof(v4) * (size_t)n);
  for (int i = 0; i < iterations; i++) {
    v4* next = cur == colA.data() ? colB.data() : colA.data();
#pragma omp parallel for
    for (int p = 0; p < n; p++)
      next[p] = dn_geometry(guide[p]) ? dn_iterate(k, cur, guide, p % width, p / width, 1 << i, side[p].w) : cur[p];
    cur = next;
  }
  if (out) for (int p = 0; p < n; p++) dn_final(cur[p], guide[p], side[p], out, p);
}

}  // namespace pt
