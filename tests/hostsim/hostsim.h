// hostsim.h -- TEST INFRASTRUCTURE.  What the translation units of libhostsim.so share: the scene a caller hands over, the host mirror of
// the device's tree, and the built scene that hostsim_create returns as a handle and every tracing entry (render, AOVs, queries, refit)
// takes.  It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#pragma once
#include <cstdint>
#include <vector>
#include "../../minimaloptix_amd/csrc/pt_path.h"
#include "../../minimaloptix_amd/csrc/pt_lbvh.h"
#include "../../minimaloptix_amd/csrc/pt_refit.h"
#include "../../minimaloptix_amd/csrc/pt_upload.h"
#include "../../minimaloptix_amd/csrc/pt_sign.h"

extern "C" {

struct hostsim_scene {
  moptix_params params;
  int32_t nMaterials; const moptix_material* materials;
  int32_t nSpheres; const moptix_sphere_params* spheres; const int32_t* sphereMat;
  int32_t nQuads; const moptix_quad_params* quads; const int32_t* quadMat;
  int32_t nLights; const moptix_light_params* lights;
  int32_t nFaces;
  const float* facePos;      // 9 floats per face: p0 p1 p2
  const float* faceNrm;      // 9 floats per face (ignored where faceHasNrm == 0); may be NULL
  const int32_t* faceHasNrm; // may be NULL
  const int32_t* faceMat;
  const float* faceUV;       // 6 floats per face (u0 v0 u1 v1 u2 v2); may be NULL
  const int32_t* faceHasUV;  // may be NULL
  int32_t nTextures; const int32_t* texSize;   // width,height per texture
  const float* const* texels;                  // nTextures pointers to 4*w*h floats
};

}  // extern "C"

namespace hostsim {

using namespace pt;

struct HostBVH {
  std::vector<Node128> nodes; std::vector<Node64> nodes64; std::vector<Tri48> tris; std::vector<TriShade> shade;
  int rootRef = kEmptyRef; int depth = 0;
  std::vector<int> levelNodes, levelLargest;      // per SAH level of the build: active nodes, the largest node's triangle count (builder 1)
};

struct HostScene {
  std::vector<DevMaterial> mats; std::vector<DevSphere> spheres; std::vector<int> sphereMat;
  std::vector<DevQuad> quads; std::vector<DevLight> lights; HostBVH bvh; SceneView view;
  std::vector<TriUV> faceUV; std::vector<DevTexture> textures;
  std::vector<std::vector<float>> texels;      // the textures' own copy of the caller's texels
};

// builder: 0 = Morton radix tree (Karras), 1 = binned SAH over the Morton order (device default)
void build_lbvh(const hostsim_scene& s, int leafSize, int builder, HostBVH& out);
void make_scene(const hostsim_scene& s, int leafSize, int builder, HostScene& hs);

// What hostsim_create returns: the scene as built, the face staging as a context keeps it, and the refit's plan (refitsim.cpp).  The
// view points into the vectors of `hs`, so a HostSim is neither copied nor moved.
struct HostSim {
  HostScene hs;
  double buildSeconds = 0.0;
  std::vector<float> facePos, faceNrm; std::vector<int> faceHasNrm;
  std::vector<RefitBox> raw;
  std::vector<int> order, levelFirst;
  bool planned = false;
  double sahCost = 0.0, sahCostBuilt = 0.0;
};

struct LocalStack {
  int data[256];
  inline void store(int sp, int v) { data[sp] = v; }
  inline int load(int sp) const { return data[sp]; }
  inline bool roomy(int) const { return true; }
  inline void store_fast(int sp, int v) { data[sp] = v; }
  static constexpr bool kFlat = false;      // pt_path.h node_step_nearfar: this stack takes the branched tail
  inline bool fits_fast(int, int) const { return false; }
  inline int peek_fast(int) const { return 0; }
};
// the point queries' entry: a reference and the squared distance to its box (pt_point.h)
struct LocalPointStack {
  int ref[256]; float d2[256];
  inline void store(int sp, int r, float d) { ref[sp] = r; d2[sp] = d; }
  inline void load(int sp, int& r, float& d) const { r = ref[sp]; d = d2[sp]; }
};

// pointsim.cpp, for signsim.cpp too: point i of a query by the traversal, and by the loop over every primitive record.  mode: POINT_CLOSEST,
// POINT_ANY (out: int32 per point) or POINT_SIGNED with the sign table (null otherwise; out: a PointHit per point)
void point_query_one(const SceneView& sc, int mode, bool n64, const SignRecord* table, const float* p, void* out, size_t i);
void point_brute_one(const SceneView& sc, int mode, const SignRecord* table, const float* p, void* out, size_t i);

// nodeFormat 64 walks the 64-byte nodes where the tree has them (as the packet kernel does by default), 128 the 128-byte ones
inline bool walks_node64(const SceneView& sc, int nodeFormat) { return nodeFormat == 64 && sc.nodes64 != nullptr; }

inline void host_trav_step(const SceneView& sc, const PathState& ps, Trav& tv, LocalStack& st, Counters& ct, bool node64) {
  if (node64) trav_step<true, true>(sc, ps, tv, st, ct); else trav_step<true, false>(sc, ps, tv, st, ct);
}

}  // namespace hostsim
