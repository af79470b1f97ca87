// querysim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the ray-query kernel (minimaloptix_amd/csrc/querykernel.hip): the same
// per-ray code (pt_query.h over pt_path.h's traversal), compiled for the host and run one ray at a time, on the scene and tree of a
// hostsim_create handle (hostsim.h).  The GPU tests compare the kernel's output with this bit for bit.  It is not part of the
// product: nothing under minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_query.h"

using namespace hostsim;

namespace {

template <bool ANY, bool N64>
void query_one(const SceneView& sc, const float* r, void* out, size_t i) {
  LocalStack st;
  Counters ct; memset(&ct, 0, sizeof(ct));
  PathState ps; memset(&ps, 0, sizeof(ps));
  Trav tv; memset(&tv, 0, sizeof(tv));
  const bool valid = query_ray(r, ps);
  query_begin<ANY>(sc, ps, valid, tv, ct);
  while (tv.node != kTravDone) query_step<ANY, N64>(sc, ps, tv, st, ct);
  if (ANY) static_cast<int32_t*>(out)[i] = tv.bestPrim >= 0 ? 1 : 0;
  else query_hit(sc, ps, tv, static_cast<QueryHit*>(out)[i]);
}

}  // namespace

extern "C" {

// moptix_query_rays on the CPU.  rays: n x 8 floats; mode 0 = closest (out: n x 32-byte hit records), 1 = any (out: n x int32).
int querysim_query(void* h, int nodeFormat, const float* rays, int64_t n, int mode, void* out) {
  if (!h || n < 0 || (n > 0 && (!rays || !out)) || (mode != QUERY_CLOSEST && mode != QUERY_ANY)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
#pragma omp parallel for schedule(dynamic, 64)
  for (int64_t i = 0; i < n; i++) {
    const float* r = rays + 8 * (size_t)i;
    if (mode == QUERY_ANY) { if (n64) query_one<true, true>(sc, r, out, (size_t)i); else query_one<true, false>(sc, r, out, (size_t)i); }
    else { if (n64) query_one<false, true>(sc, r, out, (size_t)i); else query_one<false, false>(sc, r, out, (size_t)i); }
  }
  return 0;
}

}  // extern "C"
