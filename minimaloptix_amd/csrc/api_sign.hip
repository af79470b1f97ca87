// api_sign.hip -- signed point queries (signkernel.hip, pt_sign.h, pt_signtopo.h): the topology of the uploaded faces, the table of
// pseudonormals on the device (what the signed mode of moptix_query_points* asks for, api_point.hip), moptix_get_sign_info and the test
// aid moptix_debug_read_sign_table of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "signkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(SignRecord) == 96, "moptix_debug_read_sign_table: 96 bytes per face");

namespace {

// The topology of the faces the context holds, from the host staging (device-side updates fetched back first, as moptix_build_accel does).
int ensure_topology(moptix_context c) {
  moptix_context_t::Sign& s = c->sign;
  if (s.have) return MOPTIX_OK;
  const int rc = fetch_faces(c);
  if (rc != MOPTIX_OK) return rc;
  sign_build_topology(c->facePos.data(), c->faceMat.size(), s.topo);
  s.have = true; s.uploaded = false; s.stale = true; s.tableBuilds = 0;
  return MOPTIX_OK;
}

// The device side of the topology and the table's buffers: once per topology.
int ensure_uploaded(moptix_context c) {
  moptix_context_t::Sign& s = c->sign;
  if (s.uploaded) return MOPTIX_OK;
  const SignTopology& t = s.topo;
  HIPCHK(c, s.faceIds.upload(t.faceIds, c->stream), "upload sign topology");
  HIPCHK(c, s.vertexStart.upload(t.vertexStart, c->stream), "upload sign topology");
  HIPCHK(c, s.vertexCorner.upload(t.vertexCorner, c->stream), "upload sign topology");
  HIPCHK(c, s.edgeStart.upload(t.edgeStart, c->stream), "upload sign topology");
  HIPCHK(c, s.edgeFace.upload(t.edgeFace, c->stream), "upload sign topology");
  HIPCHK(c, s.faces.ensure((size_t)t.nFaces), "alloc sign table scratch");
  HIPCHK(c, s.vertexN.ensure((size_t)t.nVerts), "alloc sign table scratch");
  HIPCHK(c, s.edgeN.ensure((size_t)t.nEdges), "alloc sign table scratch");
  HIPCHK(c, s.table.ensure((size_t)t.nFaces), "alloc sign table");
  s.uploaded = true; s.stale = true;
  return MOPTIX_OK;
}

// The table as the faces are now: enqueued, no synchronisation, nothing allocated after the first.
int ensure_table(moptix_context c) {
  moptix_context_t::Sign& s = c->sign;
  int rc = ensure_topology(c);
  if (rc != MOPTIX_OK) return rc;
  if (s.topo.nFaces == 0) return MOPTIX_OK;
  if ((size_t)s.topo.nFaces != c->refit.facesOnDevice || s.topo.nFaces != c->bvh.nTris || !c->dFacePos.p)
    return fail(c, MOPTIX_ERR_STATE, "the device copy of the faces does not match the faces the sign topology was taken from");
  if ((rc = ensure_uploaded(c)) != MOPTIX_OK) return rc;
  if (!s.stale) return MOPTIX_OK;
  SignBuildArgs a;
  memset(&a, 0, sizeof(a));
  a.nFaces = s.topo.nFaces; a.nVerts = s.topo.nVerts; a.nEdges = s.topo.nEdges;
  a.facePos = c->dFacePos.p; a.faceIds = s.faceIds.p;
  a.vertexStart = s.vertexStart.p; a.vertexCorner = s.vertexCorner.p; a.edgeStart = s.edgeStart.p; a.edgeFace = s.edgeFace.p;
  a.faces = s.faces.p; a.vertexN = s.vertexN.p; a.edgeN = s.edgeN.p; a.table = s.table.p;
  HIPCHK(c, launch_sign_table(c->stream, a), "launch sign table build");
  s.stale = false; s.tableBuilds++;
  return MOPTIX_OK;
}

}  // namespace

namespace pt { namespace api {

void sign_release(moptix_context c) {
  moptix_context_t::Sign& s = c->sign;
  if (s.uploaded && !c->poisoned) {                            // a signed query in flight still reads what is freed here
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
  }
  s.release();
}

int sign_table_for_query(moptix_context c, const SignRecord*& table) {
  const int rc = ensure_table(c);
  if (rc == MOPTIX_OK) table = c->sign.table.p;
  return rc;
}

}}  // namespace pt::api

extern "C" {

int moptix_get_sign_info(moptix_context c, moptix_sign_info* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  memset(out, 0, sizeof(*out));
  if (c->faceMat.empty()) return MOPTIX_OK;
  const int rc = ensure_topology(c);
  if (rc != MOPTIX_OK) return rc;
  const SignTopology& t = c->sign.topo;
  out->weldedVerts = (uint32_t)t.nVerts; out->edges = (uint32_t)t.nEdges;
  out->boundaryEdges = t.boundaryEdges; out->nonManifoldEdges = t.nonManifoldEdges; out->flippedEdges = t.flippedEdges;
  out->degenerateFaces = t.degenerateFaces; out->closed = t.closed() ? 1u : 0u;
  out->tableBuilds = c->sign.tableBuilds; out->signedVolume = t.signedVolume;
  return MOPTIX_OK;
}

int moptix_debug_read_sign_table(moptix_context c, void* table) {
  if (!c || !table) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  if ((rc = ensure_table(c)) != MOPTIX_OK) return rc;
  if (c->sign.topo.nFaces == 0) return MOPTIX_OK;
  return read_back(c, { { table, c->sign.table.p, sizeof(SignRecord) * (size_t)c->sign.topo.nFaces } }, "read sign table");
}

}  // extern "C"
