// signsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the signed point queries (minimaloptix_amd/csrc/signkernel.hip, api_sign.hip): the
// topology of the handle's faces (pt_signtopo.h, the function the library runs), the table of pseudonormals computed by the same per-face,
// per-vertex and per-edge code (pt_sign.h) one element at a time, and with that table the signed mode of pointsim.cpp's traversal and of
// its loop over every primitive, on the scene and tree of a hostsim_create handle (hostsim.h), through a sign state made on that handle
// (signsim_create).  The GPU tests compare the device's table and output with these bit for bit.
// It is not part of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_signtopo.h"

using namespace hostsim;

namespace {

// What signsim_create returns: the scene handle it was made on and the topology of that handle's faces, taken from the face staging as it
// is at that call (a context's first signed query).  It lives beside the scene handle and must be freed before it.
struct SignSim { HostSim* sim; SignTopology topo; std::vector<SignRecord> table; };

// The table is computed from the staging as it is NOW at every call, which is what a context's table is after its stale flag was honoured.
SignSim& refreshed(void* h) {
  SignSim& s = *static_cast<SignSim*>(h);
  const HostSim& r = *s.sim;
  const SignTopology& t = s.topo;
  std::vector<SignFace> faces((size_t)t.nFaces);
  for (int f = 0; f < t.nFaces; f++) faces[f] = sign_face(&r.facePos[9 * (size_t)f], t.faceIds[6 * (size_t)f] < 0);
  std::vector<v4> vertexN((size_t)t.nVerts), edgeN((size_t)t.nEdges);
  for (int i = 0; i < t.nVerts; i++) {
    const v3 n = sign_vertex_sum(faces.data(), t.vertexCorner.data(), t.vertexStart[i], t.vertexStart[i + 1]);
    vertexN[i] = mk4(n.x, n.y, n.z, 0.f);
  }
  for (int e = 0; e < t.nEdges; e++) {
    const v3 n = sign_edge_sum(faces.data(), t.edgeFace.data(), t.edgeStart[e], t.edgeStart[e + 1]);
    edgeN[e] = mk4(n.x, n.y, n.z, 0.f);
  }
  s.table.resize((size_t)t.nFaces);
  for (int f = 0; f < t.nFaces; f++) s.table[f] = sign_record(&t.faceIds[6 * (size_t)f], faces[f], vertexN.data(), edgeN.data());
  return s;
}

}  // namespace

extern "C" {

struct signsim_info {      // moptix_sign_info
  uint32_t weldedVerts, edges, boundaryEdges, nonManifoldEdges, flippedEdges, degenerateFaces, closed, tableBuilds;
  double signedVolume;
};

// The sign state of a hostsim_create handle: its topology, taken now.  Every entry below takes what this returns.
void* signsim_create(void* h) {
  if (!h) return nullptr;
  SignSim* s = new SignSim();
  s->sim = static_cast<HostSim*>(h);
  sign_build_topology(s->sim->facePos.data(), s->sim->facePos.size() / 9, s->topo);
  return s;
}
void signsim_free(void* s) { delete static_cast<SignSim*>(s); }

// moptix_get_sign_info (tableBuilds: 0, the mirror keeps no table)
int signsim_info_read(void* h, signsim_info* out) {
  if (!h || !out) return -1;
  memset(out, 0, sizeof(*out));
  const SignTopology& t = static_cast<SignSim*>(h)->topo;
  if (t.nFaces == 0) return 0;
  out->weldedVerts = (uint32_t)t.nVerts; out->edges = (uint32_t)t.nEdges;
  out->boundaryEdges = t.boundaryEdges; out->nonManifoldEdges = t.nonManifoldEdges; out->flippedEdges = t.flippedEdges;
  out->degenerateFaces = t.degenerateFaces; out->closed = t.closed() ? 1u : 0u; out->signedVolume = t.signedVolume;
  return 0;
}

// The table for the face staging as it is: nFaces x 96 bytes.  ids (may be NULL): nFaces x 6 int32, the topology's welded vertex and edge ids.
int signsim_table(void* h, void* table, int32_t* ids) {
  if (!h || !table) return -1;
  const SignSim& s = refreshed(h);
  if (!s.table.empty()) memcpy(table, s.table.data(), s.table.size() * sizeof(SignRecord));
  if (ids && !s.topo.faceIds.empty()) memcpy(ids, s.topo.faceIds.data(), s.topo.faceIds.size() * sizeof(int));
  return 0;
}

// moptix_query_points_device, mode MOPTIX_POINT_SIGNED, on the CPU.  points: n x 4 floats; out: n x 32-byte records.
int signsim_query(void* h, int nodeFormat, const float* points, int64_t n, void* out) {
  if (!h || n < 0 || (n > 0 && (!points || !out))) return -1;
  const SignSim& s = refreshed(h);
  const SignRecord* table = s.table.data();
  const SceneView& sc = s.sim->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) point_query_one(sc, POINT_SIGNED, n64, table, points + 4 * (size_t)i, out, (size_t)i);
  return 0;
}

// The same answers from a plain loop over every primitive record.
int signsim_brute(void* h, const float* points, int64_t n, void* out) {
  if (!h || n < 0 || (n > 0 && (!points || !out))) return -1;
  const SignSim& s = refreshed(h);
  const SignRecord* table = s.table.data();
  const SceneView& sc = s.sim->hs.view;
#pragma omp parallel for schedule(dynamic, 16)
  for (int64_t i = 0; i < n; i++) point_brute_one(sc, POINT_SIGNED, table, points + 4 * (size_t)i, out, (size_t)i);
  return 0;
}

void signsim_atan2(const float* y, const float* x, float* out, int n) {
  for (int i = 0; i < n; i++) out[i] = atan2_ac(y[i], x[i]);
}

}  // extern "C"
