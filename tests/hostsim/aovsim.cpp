// aovsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of the AOV kernel (minimaloptix_amd/csrc/aovkernel.hip): the same per-pixel
// code (pt_aov.h over pt_path.h's camera ray and traversal), compiled for the host and run one pixel at a time, on the scene and
// tree of a hostsim_create handle (hostsim.h).  The GPU tests compare the kernel's buffers with these bit for bit.  It is not part
// of the product: nothing under minimaloptix_amd/ builds or loads it.
#include <cstring>
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_aov.h"

using namespace hostsim;

extern "C" {

// host copy of a context's AOV state: the buffers of moptix_aov_read (W*H*3 floats albedo / normal, W*H floats depth / hits, W*H int32
// primId / matId; zeroed and -1 after a clear) and the number of seeds added since the clear
struct aovsim_buffers {
  float *albedo, *normal, *depth, *hits; int32_t *primId, *matId;
  uint64_t samples;
};

}  // extern "C"

namespace {

template <bool N64>
void aov_pixel(const SceneView& sc, int pix, const int32_t* seeds, int n, bool writeIds, aovsim_buffers* b) {
  LocalStack st;
  Counters ct; memset(&ct, 0, sizeof(ct));
  AovPixel acc;
  acc.albedo = mk3(b->albedo[3 * pix], b->albedo[3 * pix + 1], b->albedo[3 * pix + 2]);
  acc.normal = mk3(b->normal[3 * pix], b->normal[3 * pix + 1], b->normal[3 * pix + 2]);
  acc.depth = b->depth[pix]; acc.hits = b->hits[pix]; acc.prim = b->primId[pix]; acc.mat = b->matId[pix];
  for (int s = 0; s < n; s++) {
    PathState ps; memset(&ps, 0, sizeof(ps));
    Trav tv; memset(&tv, 0, sizeof(tv));
    ps.pixel = pix;
    begin_sample<false>(sc, ps, seeds[s], ct);
    trav_begin<false>(sc, ps, tv, ct);
    while (tv.node != kTravDone) trav_step<false, N64>(sc, ps, tv, st, ct);
    AovSample smp;
    aov_sample(sc, ps, tv, smp);
    aov_add(acc, smp, writeIds && s == 0);
  }
  b->albedo[3 * pix] = acc.albedo.x; b->albedo[3 * pix + 1] = acc.albedo.y; b->albedo[3 * pix + 2] = acc.albedo.z;
  b->normal[3 * pix] = acc.normal.x; b->normal[3 * pix + 1] = acc.normal.y; b->normal[3 * pix + 2] = acc.normal.z;
  b->depth[pix] = acc.depth; b->hits[pix] = acc.hits; b->primId[pix] = acc.prim; b->matId[pix] = acc.mat;
}

}  // namespace

extern "C" {

// moptix_render_aovs on the CPU: adds one sample per seed to every pixel of the whole frame.
int aovsim_render_aovs(void* h, int nodeFormat, const int32_t* seeds, int n, aovsim_buffers* b) {
  if (!h || !b || n < 0 || (n > 0 && !seeds)) return -1;
  const SceneView& sc = static_cast<HostSim*>(h)->hs.view;
  const bool n64 = walks_node64(sc, nodeFormat);
  const bool writeIds = b->samples == 0;
  const int nPix = sc.width * sc.height;
#pragma omp parallel for schedule(dynamic, 64)
  for (int pix = 0; pix < nPix; pix++) {
    if (n64) aov_pixel<true>(sc, pix, seeds, n, writeIds, b);
    else aov_pixel<false>(sc, pix, seeds, n, writeIds, b);
  }
  b->samples += (uint64_t)n;
  return 0;
}

// begin_sample's primary rays of one seed in moptix_debug_trace's layout: rays[8 * pixel ..] = o, d, tmin, tmax
int aovsim_camera_rays(const hostsim_scene* s, int32_t seed, float* rays) {
  if (!s || !rays) return -1;
  SceneView sc; memset(&sc, 0, sizeof(sc));
  sc.width = (int)s->params.width; sc.height = (int)s->params.height;
  sc.epsT = s->params.rayEpsilonT; sc.cam = make_cam(s->params.cam);
  Counters ct; memset(&ct, 0, sizeof(ct));
  for (int pix = 0; pix < sc.width * sc.height; pix++) {
    PathState ps; memset(&ps, 0, sizeof(ps));
    ps.pixel = pix;
    begin_sample<false>(sc, ps, seed, ct);
    float* r = rays + 8 * (size_t)pix;
    r[0] = ps.o.x; r[1] = ps.o.y; r[2] = ps.o.z; r[3] = ps.d.x; r[4] = ps.d.y; r[5] = ps.d.z; r[6] = ps.tmin; r[7] = ps.tmax;
  }
  return 0;
}

}  // extern "C"
