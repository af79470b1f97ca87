// refitkernel.hip -- in-place refit of the four-wide tree for gfx950 (definition and per-element code: pt_refit.h).
//
// Its own translation unit: nothing of it is compiled into the builder's or the trace kernels' code objects (tools/isa_diff.py).
//
//   k_refit_tris    one lane per sorted triangle slot: the face index from the old record, 36 B of positions (and of normals) gathered, the
//                   two 48-byte records written as three 16-byte stores each, the raw box as two; the scene box as lbvh.hip's k_bounds
//                   folds it (wave min / max, one lane's atomics on replicated targets, k_refit_box_fold afterwards).
//   k_refit_level   one lane per node of one level of the plan, deepest level first: a leaf child pads and unions its triangles' raw
//                   boxes (the padding needs the folded scene box, hence here and not in the triangle pass), a node child unions the box
//                   rows of the child node, which an earlier launch finished; the lane writes the whole Node128 and its Node64.
//                   Launch boundaries order the levels: no arrival counters, no fences, no agent-scope accesses.
//   k_refit_cost    the surface-area cost: one binary64 term per node, one partial sum per workgroup (a fixed tree in LDS), folded by one
//                   wave in a fixed order -- the same bits on every run.
// lbvh.hip's SceneBox helpers live in its anonymous namespace; the few lines are repeated here rather than moved, so that the builder's code
// object stays bit for bit what it was.
#include <hip/hip_runtime.h>

#include "refitkernel.h"

namespace pt {

namespace {

constexpr int kBlock = 256;
constexpr int kLevelBlock = 64;          // one wave per workgroup: the upper levels' few nodes spread over the CUs
inline int grid_for(int n, int block) { return (n + block - 1) / block; }

__global__ void k_refit_box_init(uint32_t* box) {        // <<<kRefitBoxReplicas, 64>>>
  if (threadIdx.x < kRefitBoxWords) box[blockIdx.x * kRefitBoxWords + threadIdx.x] = float_to_ordered(threadIdx.x < 3 ? 1e37f : -1e37f);
}
__global__ void k_refit_box_fold(uint32_t* box) {        // <<<1, 64>>>
  const int w = threadIdx.x;
  if (w >= kRefitBoxWords) return;
  uint32_t v = box[w];
  for (int r = 1; r < kRefitBoxReplicas; r++) { const uint32_t x = box[r * kRefitBoxWords + w]; v = w < 3 ? min(v, x) : max(v, x); }
  box[w] = v;
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf_(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf_(v, __shfl_xor(v, o));
  return v;
}

__global__ void __launch_bounds__(kBlock) k_refit_tris(const RefitArgs a) {
  const int k = blockIdx.x * kBlock + threadIdx.x;
  float l[3] = { 1e37f, 1e37f, 1e37f }, h[3] = { -1e37f, -1e37f, -1e37f };
  if (k < a.nTris) {
    Tri48 old;
    old.mat = a.tris[k].mat; old.prim = a.tris[k].prim; old.shadow = a.tris[k].shadow;
    const int f = old.prim;
    const bool hasNrm = a.faceNrm != nullptr && a.faceHasNrm != nullptr && a.faceHasNrm[f] != 0;
    Tri48 t; TriShade sh; RefitBox raw;
    refit_triangle(a.facePos + 9 * (size_t)f, a.faceNrm + 9 * (size_t)f, hasNrm, old, t, sh, raw);
    a.tris[k] = t; a.shade[k] = sh; *tri_face_slot(a.shade, a.nTris, k) = make_tri_face(t, sh); a.raw[k] = raw;
    l[0] = raw.lox; l[1] = raw.loy; l[2] = raw.loz; h[0] = raw.hix; h[1] = raw.hiy; h[2] = raw.hiz;
  }
  const float v[6] = { wave_min(l[0]), wave_min(l[1]), wave_min(l[2]), wave_max(h[0]), wave_max(h[1]), wave_max(h[2]) };
  if ((threadIdx.x & 63) == 0) {
    uint32_t* box = a.sceneBox + (blockIdx.x % kRefitBoxReplicas) * kRefitBoxWords;
    for (int i = 0; i < 3; i++) { atomicMin(&box[i], float_to_ordered(v[i])); atomicMax(&box[3 + i], float_to_ordered(v[3 + i])); }
  }
}

__device__ __forceinline__ float scene_pad_abs(const uint32_t* box) {
  return refit_pad_abs(mk3(ordered_to_float(box[0]), ordered_to_float(box[1]), ordered_to_float(box[2])),
                       mk3(ordered_to_float(box[3]), ordered_to_float(box[4]), ordered_to_float(box[5])));
}

__global__ void __launch_bounds__(kLevelBlock) k_refit_level(const RefitArgs a, int first, int count) {
  const int i = blockIdx.x * kLevelBlock + threadIdx.x;
  if (i >= count) return;
  const int n = a.levelOrder[first + i];
  const float padAbs = scene_pad_abs(a.sceneBox);
  Node128 nd = a.nodes[n];
  refit_node(nd, a.raw, padAbs, a.nodes);
  a.nodes[n] = nd;
  if (a.nodes64 != nullptr) {
    Node64 c;
    if (compress_node(nd, c)) a.nodes64[n] = c;
    else atomicAdd(a.bad, 1);      // the whole array is dropped after the refit (api_refit.hip)
  }
}

__global__ void __launch_bounds__(kBlock) k_refit_cost(const RefitArgs a) {
  __shared__ double s[kBlock];
  const int n = blockIdx.x * kBlock + threadIdx.x;
  s[threadIdx.x] = n < a.nNodes ? refit_node_cost(a.nodes[n]) : 0.0;
  __syncthreads();
  for (int o = kBlock / 2; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s[0];
}
__global__ void __launch_bounds__(64) k_refit_cost_fold(const RefitArgs a, int nPartials) {      // <<<1, 64>>>
  __shared__ double s[64];
  double v = 0.0;
  for (int i = threadIdx.x; i < nPartials; i += 64) v += a.partials[i];
  s[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 64; i++) t += s[i];
    a.cost->sum = t; a.cost->rootArea = refit_root_area(a.nodes[0]);
  }
}

__global__ void k_refit_copy_normals(int nFaces, const float* __restrict__ src, const int* __restrict__ faceHasNrm, float* __restrict__ dst) {
  const unsigned int n9 = 9u * (unsigned int)nFaces;        // one lane per float: nFaces < 2^28, so 9 * nFaces < 2^32
  const unsigned int u = (unsigned int)blockIdx.x * blockDim.x + threadIdx.x;
  if (u < n9 && faceHasNrm[u / 9u] != 0) dst[u] = src[u];
}

}  // namespace

int refit_cost_blocks(int nNodes) { return grid_for(nNodes > 0 ? nNodes : 1, kBlock); }

hipError_t launch_refit_triangles(hipStream_t stream, const RefitArgs& a) {
  if (a.nTris <= 0) return hipSuccess;
  k_refit_box_init<<<kRefitBoxReplicas, 64, 0, stream>>>(a.sceneBox);
  k_refit_tris<<<grid_for(a.nTris, kBlock), kBlock, 0, stream>>>(a);
  k_refit_box_fold<<<1, 64, 0, stream>>>(a.sceneBox);
  return hipGetLastError();
}

hipError_t launch_refit_level(hipStream_t stream, const RefitArgs& a, int first, int count) {
  if (count <= 0) return hipSuccess;
  k_refit_level<<<grid_for(count, kLevelBlock), kLevelBlock, 0, stream>>>(a, first, count);
  return hipGetLastError();
}

hipError_t launch_refit_cost(hipStream_t stream, const RefitArgs& a) {
  if (a.nNodes <= 0) return hipSuccess;
  const int blocks = refit_cost_blocks(a.nNodes);
  k_refit_cost<<<blocks, kBlock, 0, stream>>>(a);
  k_refit_cost_fold<<<1, 64, 0, stream>>>(a, blocks);
  return hipGetLastError();
}

hipError_t launch_refit_copy_normals(hipStream_t stream, int nFaces, const float* src, const int* faceHasNrm, float* dst) {
  if (nFaces <= 0) return hipSuccess;
  const unsigned int n9 = 9u * (unsigned int)nFaces;
  k_refit_copy_normals<<<(n9 + kBlock - 1) / kBlock, kBlock, 0, stream>>>(nFaces, src, faceHasNrm, dst);
  return hipGetLastError();
}

}  // namespace pt
