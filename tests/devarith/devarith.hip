// devarith.hip -- the device side of the arithmetic contract tests (test infrastructure; tests/devarith_helpers.py, tests/test_gpu_devarith.py).
//
// One element-wise kernel per primitive of devarith_ops.h: one thread per element, grid = ceil(n / 256), plain loads and stores.  The
// kernels are the product headers' functions compiled ALONE with the product's flags (the top Makefile hands its HIPFLAGS down): they pin
// the primitives, not the product kernels' instruction streams.  Inputs and outputs are arrays of n floats per operand, one after the
// other ([NIN][n] and [NOUT][n]).  The launchers take host pointers, do their own allocation and copies, launch ONCE, and return the HIP
// error code.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../minimaloptix_amd/csrc/pt_lanestack.h"

#define DA_OP(name, NIN, NOUT, ...)                                                                         \
  __global__ void da_kernel_##name(const float* __restrict__ in, float* __restrict__ out, long n) {         \
    const long i = (long)blockIdx.x * 256 + threadIdx.x;                                                    \
    if (i >= n) return;                                                                                     \
    float x[NIN], y[NOUT];                                                                                  \
    for (int k = 0; k < NIN; k++) x[k] = in[(size_t)k * n + i];                                             \
    __VA_ARGS__                                                                                             \
    for (int k = 0; k < NOUT; k++) out[(size_t)k * n + i] = y[k];                                           \
  }
#define DA_DEVICE_OP DA_OP
#include "devarith_ops.h"
#undef DA_OP
#undef DA_DEVICE_OP

__global__ void da_kernel_tex2d(pt::DevTexture t, const float* __restrict__ uv, float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const pt::v4 r = pt::tex2d(t, uv[i], uv[(size_t)n + i]);
  out[i] = r.x; out[(size_t)n + i] = r.y; out[(size_t)2 * n + i] = r.z; out[(size_t)3 * n + i] = r.w;
}

namespace {
struct Row { const char* name; int nin, nout; void (*kernel)(const float*, float*, long); };
#define DA_OP(name, NIN, NOUT, ...) { #name, NIN, NOUT, da_kernel_##name },
#define DA_DEVICE_OP DA_OP
const Row kRows[] = {
#include "devarith_ops.h"
};
#undef DA_OP
#undef DA_DEVICE_OP

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};
#define DA_TRY(e) do { const hipError_t err_ = (e); if (err_ != hipSuccess) return (int)err_; } while (0)
unsigned grid_of(long n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" {

// number of operand arrays a primitive reads / writes; -1: no such primitive
int da_dev_arity(const char* name, int* nin, int* nout) {
  for (const Row& r : kRows)
    if (!strcmp(r.name, name)) { *nin = r.nin; *nout = r.nout; return 0; }
  return -1;
}

// in: [nin][n] floats, out: [nout][n] floats, host memory.  Returns the HIP error code, -1 for an unknown name, -2 for n out of range.
int da_dev_run(const char* name, const float* in, float* out, long n) {
  const Row* row = nullptr;
  for (const Row& r : kRows)
    if (!strcmp(r.name, name)) row = &r;
  if (!row) return -1;
  if (n <= 0 || n > (1L << 26)) return -2;
  DevBuf din, dout;
  const size_t inBytes = (size_t)row->nin * n * sizeof(float), outBytes = (size_t)row->nout * n * sizeof(float);
  DA_TRY(hipMalloc(&din.p, inBytes));
  DA_TRY(hipMalloc(&dout.p, outBytes));
  DA_TRY(hipMemcpy(din.p, in, inBytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(row->kernel, dim3(grid_of(n)), dim3(256), 0, 0, (const float*)din.p, (float*)dout.p, n);
  DA_TRY(hipGetLastError());
  DA_TRY(hipDeviceSynchronize());
  DA_TRY(hipMemcpy(out, dout.p, outBytes, hipMemcpyDeviceToHost));
  return 0;
}

// texels: [height][width][4] floats; uv: [2][n]; out: [4][n].  Every index tex2d forms is in range by tex_wrap for any int.
int da_dev_tex2d(const float* texels, int width, int height, const float* uv, float* out, long n) {
  if (n <= 0 || n > (1L << 26) || width < 1 || height < 1) return -2;
  DevBuf dtex, duv, dout;
  const size_t texBytes = (size_t)width * height * 4 * sizeof(float);
  DA_TRY(hipMalloc(&dtex.p, texBytes));
  DA_TRY(hipMalloc(&duv.p, (size_t)2 * n * sizeof(float)));
  DA_TRY(hipMalloc(&dout.p, (size_t)4 * n * sizeof(float)));
  DA_TRY(hipMemcpy(dtex.p, texels, texBytes, hipMemcpyHostToDevice));
  DA_TRY(hipMemcpy(duv.p, uv, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice));
  pt::DevTexture t; t.texels = (const pt::v4*)dtex.p; t.width = width; t.height = height;
  hipLaunchKernelGGL(da_kernel_tex2d, dim3(grid_of(n)), dim3(256), 0, 0, t, (const float*)duv.p, (float*)dout.p, n);
  DA_TRY(hipGetLastError());
  DA_TRY(hipDeviceSynchronize());
  DA_TRY(hipMemcpy(out, dout.p, (size_t)4 * n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"
