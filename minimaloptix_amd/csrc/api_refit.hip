// api_refit.hip -- mesh vertex updates and the in-place refit (refitkernel.hip, pt_refit.h): the moptix_update_faces*, moptix_refit_accel
// and moptix_get_refit_info entry points of include/moptix.h.
#include <cmath>
#include <cstring>

#include "api_context.h"

using namespace pt;
using namespace pt::api;

namespace {

int check_update(moptix_context c, int32_t first, int32_t n, const float* pos) {
  if (!c) return fail(nullptr, MOPTIX_ERR_INVALID, "null context");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  if (first < 0 || n < 0 || (size_t)first + (size_t)n > c->faceMat.size()) return fail(c, MOPTIX_ERR_INVALID, "bad face range");
  if (n > 0 && !pos) return fail(c, MOPTIX_ERR_INVALID, "null positions");
  return MOPTIX_OK;
}

RefitArgs refit_args(moptix_context c) {
  RefitArgs a;
  memset(&a, 0, sizeof(a));
  a.nTris = c->bvh.nTris; a.nNodes = c->bvh.nNodes;
  a.tris = c->bvh.tris; a.shade = c->bvh.shade; a.nodes = c->bvh.nodes; a.nodes64 = c->bvh.nodes64;
  a.facePos = c->dFacePos.p; a.faceNrm = c->dFaceNrm.p; a.faceHasNrm = c->dFaceHasNrm.p;
  a.raw = c->refit.raw.p; a.sceneBox = c->refit.sceneBox.p; a.levelOrder = c->refit.levelOrder.p;
  a.partials = c->refit.partials.p; a.cost = c->refit.cost.p; a.bad = c->refit.bad.p;
  return a;
}

double cost_ratio(const RefitCost& k) { return k.rootArea > 0.0 ? k.sum / k.rootArea : 0.0; }

// The plan of the tree the context holds: made once, from the emitted nodes' references; the built tree's cost is taken here, before
// the first refit overwrites a box.
int ensure_plan(moptix_context c) {
  moptix_context_t::Refit& r = c->refit;
  if (r.planned) return MOPTIX_OK;
  r.drop();
  const int nNodes = c->bvh.nNodes;
  HIPCHK(c, hipEventCreate(&r.e0), "hipEventCreate"); HIPCHK(c, hipEventCreate(&r.e1), "hipEventCreate");
  HIPCHK(c, hipHostMalloc((void**)&r.pinned, sizeof(*r.pinned), hipHostMallocDefault), "alloc refit read-back");
  memset(r.pinned, 0, sizeof(*r.pinned));
  HIPCHK(c, r.raw.ensure((size_t)c->bvh.nTris), "alloc refit boxes");
  HIPCHK(c, r.sceneBox.ensure((size_t)kRefitBoxReplicas * kRefitBoxWords), "alloc refit scene box");
  HIPCHK(c, r.partials.ensure((size_t)refit_cost_blocks(nNodes)), "alloc refit cost partials");
  HIPCHK(c, r.cost.ensure(1), "alloc refit cost"); HIPCHK(c, r.bad.ensure(1), "alloc refit flag");
  HIPCHK(c, r.levelOrder.ensure((size_t)nNodes), "alloc refit plan");
  if (nNodes > 0) {
    std::vector<Node128> nodes((size_t)nNodes);
    HIPCHK(c, hipMemcpyAsync(nodes.data(), c->bvh.nodes, sizeof(Node128) * (size_t)nNodes, hipMemcpyDeviceToHost, c->stream), "read nodes for the refit plan");
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
    std::vector<int> order;
    if (!refit_plan_levels(nodes.data(), nNodes, order, r.levelFirst)) { r.drop(); return fail(c, MOPTIX_ERR_STATE, "the node references do not form a tree"); }
    HIPCHK(c, hipMemcpyAsync(r.levelOrder.p, order.data(), sizeof(int) * order.size(), hipMemcpyHostToDevice, c->stream), "upload refit plan");
    const RefitArgs a = refit_args(c);
    HIPCHK(c, launch_refit_cost(c->stream, a), "refit cost kernel");
    HIPCHK(c, hipMemcpyAsync(&r.pinned->cost, r.cost.p, sizeof(RefitCost), hipMemcpyDeviceToHost, c->stream), "read refit cost");
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync");      // `order` dies here
    r.info.sahCostBuilt = cost_ratio(r.pinned->cost);
  }
  r.info.sahCost = r.info.sahCostBuilt;
  r.info.has64 = c->bvh.nodes64 != nullptr && nNodes > 0 ? 1u : 0u;
  r.planned = true;
  return MOPTIX_OK;
}

}  // namespace

namespace pt { namespace api {

int refit_plan(moptix_context c) { return ensure_plan(c); }

// The device copy holds the faces the last moptix_build_accel uploaded: the first facesOnDevice of the staging.  moptix_add_mesh may have
// appended faces since (they exist in the staging only and are left alone); nothing but moptix_clear_scene removes faces, and that
// clears hostStale.
int fetch_faces(moptix_context c) {
  if (!c->refit.hostStale) return MOPTIX_OK;
  const size_t n9 = 9 * c->refit.facesOnDevice;
  if (n9 == 0 || n9 > c->facePos.size() || n9 > c->faceNrm.size() || !c->dFacePos.p || c->dFacePos.n < n9 || !c->dFaceNrm.p || c->dFaceNrm.n < n9)
    return fail(c, MOPTIX_ERR_STATE, "the device copy of the faces does not match the scene: the device-side face updates cannot be fetched back");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  HIPCHK(c, hipMemcpyAsync(c->facePos.data(), c->dFacePos.p, sizeof(float) * n9, hipMemcpyDeviceToHost, c->stream), "fetch face positions");
  HIPCHK(c, hipMemcpyAsync(c->faceNrm.data(), c->dFaceNrm.p, sizeof(float) * n9, hipMemcpyDeviceToHost, c->stream), "fetch face normals");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  c->refit.hostStale = false;
  return MOPTIX_OK;
}

}}  // namespace pt::api

extern "C" {

int moptix_update_faces(moptix_context c, int32_t first, int32_t n, const float* pos9, const float* nrm9) {
  int rc = check_update(c, first, n, pos9);
  if (rc != MOPTIX_OK || n == 0) return rc;
  for (size_t i = 0; i < 9 * (size_t)n; i++)
    if (!std::isfinite(pos9[i]) || (nrm9 && !std::isfinite(nrm9[i]))) return fail(c, MOPTIX_ERR_INVALID, "non-finite face position or normal");
  if ((rc = fetch_faces(c)) != MOPTIX_OK) return rc;          // a partial host update must not be overwritten by a later fetch of older data
  memcpy(c->facePos.data() + 9 * (size_t)first, pos9, sizeof(float) * 9 * (size_t)n);
  c->sign.stale = true; c->winding.stale = true;
  if (nrm9)
    for (int32_t f = 0; f < n; f++)
      if (c->faceHasNrm[first + f]) memcpy(c->faceNrm.data() + 9 * (size_t)(first + f), nrm9 + 9 * (size_t)f, sizeof(float) * 9);
  if (!c->accelBuilt) return MOPTIX_OK;                       // the staging only: moptix_build_accel uploads it
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  HIPCHK(c, hipMemcpyAsync(c->dFacePos.p + 9 * (size_t)first, c->facePos.data() + 9 * (size_t)first, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream), "update face positions");
  if (nrm9) HIPCHK(c, hipMemcpyAsync(c->dFaceNrm.p + 9 * (size_t)first, c->faceNrm.data() + 9 * (size_t)first, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice, c->stream), "update face normals");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  c->refit.facesDirty = true; c->tp.faces.changed = true;
  return MOPTIX_OK;
}

int moptix_update_faces_device(moptix_context c, int32_t first, int32_t n, const float* dPos9, const float* dNrm9) {
  int rc = check_update(c, first, n, dPos9);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((reinterpret_cast<uintptr_t>(dPos9) & 3u) != 0 || (reinterpret_cast<uintptr_t>(dNrm9) & 3u) != 0)
    return fail(c, MOPTIX_ERR_INVALID, "misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  const size_t bytes = sizeof(float) * 9 * (size_t)n;
  c->sign.stale = true; c->winding.stale = true;
  if (!c->accelBuilt) {                                       // no device copy of the faces yet: into the staging, now
    if ((rc = fetch_faces(c)) != MOPTIX_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
    HIPCHK(c, hipMemcpy(c->facePos.data() + 9 * (size_t)first, dPos9, bytes, hipMemcpyDeviceToHost), "fetch face positions");
    if (dNrm9) {
      std::vector<float> nrm(9 * (size_t)n);
      HIPCHK(c, hipMemcpy(nrm.data(), dNrm9, bytes, hipMemcpyDeviceToHost), "fetch face normals");
      for (int32_t f = 0; f < n; f++)
        if (c->faceHasNrm[first + f]) memcpy(c->faceNrm.data() + 9 * (size_t)(first + f), nrm.data() + 9 * (size_t)f, sizeof(float) * 9);
    }
    return MOPTIX_OK;
  }
  HIPCHK(c, hipMemcpyAsync(c->dFacePos.p + 9 * (size_t)first, dPos9, bytes, hipMemcpyDeviceToDevice, c->stream), "update face positions");
  if (dNrm9) HIPCHK(c, launch_refit_copy_normals(c->stream, n, dNrm9, c->dFaceHasNrm.p + first, c->dFaceNrm.p + 9 * (size_t)first), "update face normals");
  c->refit.facesDirty = true; c->refit.hostStale = true; c->tp.faces.changed = true;
  return MOPTIX_OK;
}

int moptix_refit_accel(moptix_context c) {
  if (!c) return fail(nullptr, MOPTIX_ERR_INVALID, "null context");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  if (!c->accelBuilt) return fail(c, MOPTIX_ERR_STATE, "moptix_build_accel has not been called since the scene changed: there is no tree to refit");
  int rc = begin_call(c, false);
  if (rc != MOPTIX_OK) return rc;
  if (c->bvh.nTris <= 0) { c->refit.facesDirty = false; return MOPTIX_OK; }
  if ((rc = ensure_plan(c)) != MOPTIX_OK) return rc;
  moptix_context_t::Refit& r = c->refit;
  const RefitArgs a = refit_args(c);
  r.pinned->bad = 0;
  HIPCHK(c, hipEventRecord(r.e0, c->stream), "event");
  HIPCHK(c, hipMemsetAsync(r.bad.p, 0, sizeof(int), c->stream), "clear refit flag");
  HIPCHK(c, launch_refit_triangles(c->stream, a), "refit triangle kernel");
  for (size_t L = r.levelFirst.size(); L-- > 1;)               // deepest level first
    HIPCHK(c, launch_refit_level(c->stream, a, r.levelFirst[L - 1], r.levelFirst[L] - r.levelFirst[L - 1]), "refit node kernel");
  if (a.nNodes > 0) {
    HIPCHK(c, launch_refit_cost(c->stream, a), "refit cost kernel");
    HIPCHK(c, hipMemcpyAsync(&r.pinned->cost, r.cost.p, sizeof(RefitCost), hipMemcpyDeviceToHost, c->stream), "read refit cost");
    HIPCHK(c, hipMemcpyAsync(&r.pinned->bad, r.bad.p, sizeof(int), hipMemcpyDeviceToHost, c->stream), "read refit flag");
  }
  HIPCHK(c, hipEventRecord(r.e1, c->stream), "event");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  HIPCHK(c, hipGetLastError(), "refit");
  (void)hipEventElapsedTime(&r.info.refitMs, r.e0, r.e1);
  if (a.nNodes > 0) r.info.sahCost = cost_ratio(r.pinned->cost);
  if (c->bvh.nodes64 && r.pinned->bad != 0) {                  // a node grew wider than the grid can span: as at build, this tree has no 64-byte form
    (void)hipFree(c->bvh.nodes64); c->bvh.nodes64 = nullptr;
    c->formatDecided = false; c->nodeFormatUsed = 128;
  }
  r.info.has64 = c->bvh.nodes64 != nullptr && a.nNodes > 0 ? 1u : 0u;
  r.facesDirty = false; c->sign.stale = true; c->winding.stale = true;
  return MOPTIX_OK;
}

int moptix_get_refit_info(moptix_context c, moptix_refit_info* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  *out = c->refit.info;
  return MOPTIX_OK;
}

int moptix_debug_buffer_addresses(moptix_context c, uint64_t out[8]) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  const moptix_context_t::Refit& r = c->refit;
  const void* p[8] = { c->query.overflow.p, r.levelOrder.p, r.raw.p, r.sceneBox.p, r.partials.p, r.cost.p, r.bad.p, r.pinned };
  for (int i = 0; i < 8; i++) out[i] = (uint64_t)reinterpret_cast<uintptr_t>(p[i]);
  return MOPTIX_OK;
}

}  // extern "C"
