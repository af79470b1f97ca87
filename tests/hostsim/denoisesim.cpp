// denoisesim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the denoiser kernels (minimaloptix_amd/csrc/denoisekernel.hip): the same
// per-pixel code (pt_denoise.h), compiled for the host and run pass by pass over caller-given float arrays, in the order the kernels
// run it (atrous_host.h, which temporalsim shares).  The GPU tests compare the kernels' output with this bit for bit.  It is not part of
// the product: nothing under minimaloptix_amd/ builds or loads it.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/moptix.h"
#include "atrous_host.h"

using namespace pt;

extern "C" {

// moptix_denoise on the CPU over host arrays in the accumulation buffer's layout (row 0 = bottom): accum, albedo, normal W*H*3
// floats, depth, hits W*H floats; nSamples = moptix_aov_samples.  out: W*H*3 floats.  Parameters are taken as given (the C ABI
// checks their ranges).
int denoisesim_run(int width, int height, const float* accum, const float* albedo, const float* normal, const float* depth,
                   const float* hits, float nAccumulation, float nSamples, const moptix_denoise_params* prm, float* out) {
  if (width <= 0 || height <= 0 || !accum || !albedo || !normal || !depth || !hits || !prm || !out) return -1;
  const int n = width * height;
  DenoiseConsts k;
  k.width = width; k.height = height; k.normalPower = prm->normalPower;
  k.sigmaLuminance = prm->sigmaLuminance; k.sigmaDepth = prm->sigmaDepth;
  const int demodulate = prm->iterations > 0 ? prm->demodulate : 0;
  std::vector<v4> colA(n), colB(n), guide(n), side(n);
#pragma omp parallel for
  for (int p = 0; p < n; p++) dn_decode(accum, albedo, normal, depth, hits, nAccumulation, nSamples, demodulate, p, colA[p], guide[p], side[p]);
  atrous_host(k, colA, colB, guide.data(), side.data(), prm->iterations, false, nullptr, out);
  return 0;
}

// exp_ac and pow_int_ac element-wise (for the tests of the arithmetic itself)
void denoisesim_exp_ac(const float* x, float* y, int n) {
  for (int i = 0; i < n; i++) y[i] = exp_ac(x[i]);
}
void denoisesim_pow_int(const float* x, int e, float* y, int n) {
  for (int i = 0; i < n; i++) y[i] = pow_int_ac(x[i], e);
}

}  // extern "C"
