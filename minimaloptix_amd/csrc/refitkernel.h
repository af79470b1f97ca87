// refitkernel.h -- launchers of the in-place refit (refitkernel.hip; per-element code: pt_refit.h)
#pragma once
#include <hip/hip_runtime.h>
#include "pt_refit.h"

namespace pt {

constexpr int kRefitBoxReplicas = 64;          // replicas of the scene box's atomic targets (lbvh.hip kReplicas: why)
constexpr int kRefitBoxWords = 6;              // sLo xyz, sHi xyz as order-preserving uints
struct RefitCost { double sum, rootArea; };    // refit_node_cost over all nodes; refit_root_area

struct RefitArgs {
  int nTris, nNodes;
  Tri48* tris; TriShade* shade; Node128* nodes; Node64* nodes64;      // the tree (nodes64 may be null)
  const float* facePos; const float* faceNrm; const int* faceHasNrm;  // per face in upload order (faceNrm / faceHasNrm may be null)
  RefitBox* raw;                     // nTris: the raw boxes by sorted slot
  uint32_t* sceneBox;                // kRefitBoxReplicas x kRefitBoxWords
  const int* levelOrder;             // nNodes: the plan's node order (pt_refit.h refit_plan_levels)
  double* partials;                  // one per workgroup of the cost kernel: refit_cost_blocks(nNodes)
  RefitCost* cost;                   // device: the folded cost
  int* bad;                          // device: nodes whose 64-byte form does not exist after this refit
};

int refit_cost_blocks(int nNodes);
// The triangle pass: records and raw boxes of every slot, and the scene box folded into replica 0.
hipError_t launch_refit_triangles(hipStream_t stream, const RefitArgs& a);
// One level of the node pass: the nodes levelOrder[first .. first + count).  Deepest level first.
hipError_t launch_refit_level(hipStream_t stream, const RefitArgs& a, int first, int count);
// The cost of the tree as it stands, into a.cost (a.partials is its scratch).
hipError_t launch_refit_cost(hipStream_t stream, const RefitArgs& a);
// moptix_update_faces_device's copy of normals: only into faces that have normals.
hipError_t launch_refit_copy_normals(hipStream_t stream, int nFaces, const float* src, const int* faceHasNrm, float* dst);

}  // namespace pt
