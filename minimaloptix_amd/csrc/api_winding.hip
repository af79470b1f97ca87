// api_winding.hip -- winding-number queries (windingkernel.hip, pt_winding.h): the table of cluster moments on the device and the
// moptix_query_winding*, moptix_get_winding_info and moptix_debug_read_winding_table entry points of include/moptix.h.
#include <cstring>

#include "api_context.h"
#include "windingkernel.h"

using namespace pt;
using namespace pt::api;

static_assert(sizeof(WindingNode) == 128, "moptix_debug_read_winding_table: 128 bytes per node");

namespace {

bool misaligned(const void* p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

int check_winding(moptix_context c, const float* points, int64_t n, const float* out) {
  const int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (n < 0) return fail(c, MOPTIX_ERR_INVALID, "bad point count");
  if (n > 0 && (!points || !out)) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  return MOPTIX_OK;
}

// The table as the tree is now: one launch per level of the refit's plan, deepest first, enqueued on the context's stream.  The plan
// is made here where no refit has made it yet (that reads the nodes back once per built tree: the one host synchronisation of a
// winding query, at the first after a build); nothing is allocated or launched after the first while the table is not stale.
int ensure_table(moptix_context c) {
  moptix_context_t::Winding& w = c->winding;
  const int nNodes = c->bvh.nNodes;
  if (nNodes <= 0) return MOPTIX_OK;
  if (!w.stale && w.table.p) return MOPTIX_OK;
  if (nNodes > kWindingMaxNodes) return fail(c, MOPTIX_ERR_INVALID, "winding-number queries index the moments table with 32-bit byte offsets: too many nodes");
  const int rc = refit_plan(c);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, w.table.ensure((size_t)nNodes), "alloc winding moments table");
  WindingTableArgs a;
  a.nodes = c->bvh.nodes; a.tris = c->bvh.tris; a.levelOrder = c->refit.levelOrder.p; a.table = w.table.p;
  const std::vector<int>& lf = c->refit.levelFirst;
  for (size_t L = lf.size(); L-- > 1;)                         // deepest level first
    HIPCHK(c, launch_winding_level(c->stream, a, lf[L - 1], lf[L] - lf[L - 1]), "launch winding moments pass");
  w.stale = false; w.tableBuilds++;
  return MOPTIX_OK;
}

// Enqueues the query on the context's stream, in launches of at most kWindingMaxLaunch points, the moments pass in front of it where the
// table is missing or stale.  The stack overflow area is the winding queries' own: allocated at the first such query after a build.
int enqueue_winding(moptix_context c, const float* dPoints, int64_t n, float* dOut) {
  const int rc = ensure_table(c);
  if (rc != MOPTIX_OK) return rc;
  WindingArgs a;
  memset(&a, 0, sizeof(a));
  const int nBlocks = fill_query_view(c, a.scene);
  a.table = c->bvh.nNodes > 0 ? c->winding.table.p : nullptr;
  const size_t ovf = a.scene.rootRef != kEmptyRef ? windingkernel_overflow_ints(nBlocks, c->bvh.stackBound) : 0;
  if (ovf > 0) {
    HIPCHK(c, c->winding.overflow.ensure(ovf), "alloc winding query stack overflow area");
    a.stackOverflow = c->winding.overflow.p;
  }
  for (int64_t first = 0; first < n; first += kWindingMaxLaunch) {
    a.points = dPoints + 4 * first;
    a.out = dOut + first;
    a.n = (int)(n - first < kWindingMaxLaunch ? n - first : kWindingMaxLaunch);
    HIPCHK(c, launch_windingquery(c->stream, a, nBlocks), "launch winding query");
  }
  return MOPTIX_OK;
}

}  // namespace

namespace pt { namespace api {

void winding_release(moptix_context c) {
  moptix_context_t::Winding& w = c->winding;
  if ((w.table.p || w.overflow.p) && !c->poisoned) {           // a winding query in flight still reads what is freed here
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
  }
  w.drop();
}

}}  // namespace pt::api

extern "C" {

int moptix_query_winding_device(moptix_context c, const float* dPoints, int64_t n, float* dOut) {
  int rc = check_winding(c, dPoints, n, dOut);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if (misaligned(dPoints, 15u) || misaligned(dOut, 3u))
    return fail(c, MOPTIX_ERR_INVALID, "winding queries read points 16 bytes at a time and write float results: misaligned device pointer");
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  return enqueue_winding(c, dPoints, n, dOut);
}

int moptix_query_winding(moptix_context c, const float* points, int64_t n, float* out) {
  int rc = check_winding(c, points, n, out);
  if (rc != MOPTIX_OK || n == 0) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  HIPCHK(c, c->winding.points.ensure(4 * (size_t)n), "alloc query points");
  HIPCHK(c, c->winding.out.ensure((size_t)n), "alloc winding query results");
  HIPCHK(c, hipMemcpyAsync(c->winding.points.p, points, sizeof(float) * 4 * (size_t)n, hipMemcpyHostToDevice, c->stream), "upload query points");
  if ((rc = enqueue_winding(c, c->winding.points.p, n, c->winding.out.p)) != MOPTIX_OK) return rc;
  return read_back(c, { { out, c->winding.out.p, sizeof(float) * (size_t)n } }, "read winding query results");
}

int moptix_get_winding_info(moptix_context c, moptix_winding_info* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (c->poisoned) return fail(c, MOPTIX_ERR_COMM, "this context is unusable: kernels of an aborted collective never left its stream");
  memset(out, 0, sizeof(*out));
  const moptix_context_t::Winding& w = c->winding;
  out->tableBuilds = w.tableBuilds;
  out->nodes = c->accelBuilt && c->bvh.nNodes > 0 ? (uint32_t)c->bvh.nNodes : 0u;
  out->tableBytes = w.table.p ? (uint64_t)(sizeof(WindingNode) * w.table.n) : 0u;
  out->stale = (w.stale || !w.table.p) ? 1u : 0u;
  return MOPTIX_OK;
}

int moptix_debug_read_winding_table(moptix_context c, void* table) {
  if (!c || !table) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if ((rc = begin_call(c, false)) != MOPTIX_OK) return rc;
  if ((rc = ensure_table(c)) != MOPTIX_OK) return rc;
  if (c->bvh.nNodes <= 0) return MOPTIX_OK;
  return read_back(c, { { table, c->winding.table.p, sizeof(WindingNode) * (size_t)c->bvh.nNodes } }, "read winding moments table");
}

}  // extern "C"
