// temporalsim.cpp -- TEST INFRASTRUCTURE.  The CPU mirror of moptix_denoise_temporal (minimaloptix_amd/csrc/temporalkernel.hip,
// facemotionkernel.hip and the history bookkeeping of api_temporal.hip): the same per-pixel and per-face code (pt_temporal.h,
// pt_denoise.h), compiled for the host and run pass by pass over caller-given float arrays, in the order the kernels run it (the
// a-trous passes: atrous_host.h), with the history kept in an object between calls.  With the option "temporal_face_motion" (off by
// default) it also keeps the face snapshot, the per-face records and the rules that decide whether the face pass runs.
// The GPU tests compare the device's output with this bit for bit.  It is not part of the product: nothing under minimaloptix_amd/
// builds or loads it.
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/moptix.h"
#include "atrous_host.h"

using namespace pt;

namespace {

struct Sim {
  std::vector<v4> col[2], guide[2], mom[2];
  int cur = 0;
  bool have = false;
  int width = 0, height = 0, nSpheres = 0, demodulate = 0;
  TpCamera cam{};
  std::vector<v3> centres;
  uint64_t frames = 0;
  // the context's option, face snapshot and "faces may have changed" flag
  int option = 0;
  bool faceHave = false, changed = true;
  std::vector<float> prev;
  std::vector<v4> rec;
  void drop() { have = false; frames = 0; faceHave = false; }
};

TpCamera to_camera(const moptix_cam_params& c) {
  TpCamera t;
  t.origin = mk3(c.origin.x, c.origin.y, c.origin.z); t.horizontal = mk3(c.horizontal.x, c.horizontal.y, c.horizontal.z);
  t.vertical = mk3(c.vertical.x, c.vertical.y, c.vertical.z);
  t.lowerLeft = mk3(c.scrLowerLeftCorner.x, c.scrLowerLeftCorner.y, c.scrLowerLeftCorner.z);
  return t;
}

}  // namespace

extern "C" {

void* temporalsim_create() { return new Sim; }
void temporalsim_destroy(void* s) { delete (Sim*)s; }
void temporalsim_reset(void* s) { ((Sim*)s)->drop(); }                                  // moptix_temporal_reset
void temporalsim_clear_scene(void* s) { ((Sim*)s)->drop(); ((Sim*)s)->changed = true; } // moptix_clear_scene
void temporalsim_faces_changed(void* s) { ((Sim*)s)->changed = true; }                  // moptix_update_faces*, moptix_build_accel
void temporalsim_set_option(void* s, int v) { ((Sim*)s)->option = v; if (!v) ((Sim*)s)->faceHave = false; }
uint64_t temporalsim_frames(void* s) { return ((Sim*)s)->frames; }

// moptix_denoise_temporal on the CPU over host arrays in the accumulation buffer's layout.  centres: nSpheres * 3 floats (the context's
// spheres now).  facePos (may be NULL with nFaces = 0): 9 floats for each of the nFaces faces on the device as they stand now; firstFace
// = nSpheres + nQuads.  Outputs, each optional: out W*H*3; motion W*H*2; history W*H; pre W*H*4 = {I_acc, v} as the first a-trous
// iteration reads them (after the prepass; before it with iterations = 0); counters[4] = geometry, history, disoccluded pixels, sum
// of h over the geometry pixels; faceStats[3] = tracked faces, moved faces, moved pixels.  Parameters are taken as given (the C ABI
// checks their ranges).
int temporalsim_run(void* state, int width, int height, const float* accum, const float* albedo, const float* normal, const float* depth,
                    const float* hits, const int32_t* primId, const int32_t* matId, float nAccumulation, float nSamples,
                    const moptix_cam_params* cam, const float* centres, int nSpheres, const float* facePos, int nFaces, int firstFace,
                    const moptix_denoise_params* prm, const moptix_temporal_params* tprm, float* out, float* motionOut, float* historyOut,
                    float* pre, uint64_t* counters, uint64_t* faceStats) {
  Sim* s = (Sim*)state;
  if (!s || width <= 0 || height <= 0 || !accum || !albedo || !normal || !depth || !hits || !primId || !matId || !cam || !prm || !tprm ||
      (nSpheres > 0 && !centres) || nFaces < 0 || (nFaces > 0 && !facePos))
    return -1;
  const int n = width * height;
  const int demodulate = prm->iterations > 0 ? prm->demodulate : 0;
  if (!tp_history_kept(s->have, s->width, s->height, s->nSpheres, s->demodulate, width, height, nSpheres, demodulate)) s->drop();
  DenoiseConsts k;
  k.width = width; k.height = height; k.normalPower = prm->normalPower;
  k.sigmaLuminance = prm->sigmaLuminance; k.sigmaDepth = prm->sigmaDepth;
  TemporalConsts t{};
  t.width = width; t.height = height; t.maxHistory = tprm->maxHistory; t.varianceFrames = tprm->varianceFrames;
  t.alpha = tprm->alpha; t.alphaMoments = tprm->alphaMoments; t.depthTolerance = tprm->depthTolerance; t.normalThreshold = tprm->normalThreshold;
  t.cam = to_camera(*cam);
  t.haveHistory = s->have ? 1 : 0;
  std::vector<v3> now((size_t)nSpheres);
  for (int i = 0; i < nSpheres; i++) now[i] = mk3(centres[3 * i], centres[3 * i + 1], centres[3 * i + 2]);
  std::vector<v4> motion((size_t)nSpheres);
  if (s->have) {
    tp_solve_consts(s->cam, t);
    t.sameCamera = tp_same_camera(s->cam, t.cam) ? 1 : 0;
    t.nSpheres = nSpheres;
    for (int i = 0; i < nSpheres; i++) { const v3 d = now[i] - s->centres[i]; motion[i] = mk4(d.x, d.y, d.z, 0.0f); }
  }
  // the face pass (api_temporal.hip): without a usable snapshot it only takes one; with one it runs only where the faces may have changed
  const bool on = s->option != 0;
  if (!on) { s->faceHave = false; nFaces = 0; }
  const bool tracked = on && s->faceHave && s->prev.size() == 9 * (size_t)nFaces;
  const bool facePass = on && nFaces > 0 && (!tracked || s->changed);
  uint64_t fs[3] = { tracked ? (uint64_t)nFaces : 0, 0, 0 };
  TpFaces faces{};
  if (facePass) {
    s->rec.assign(3 * (size_t)nFaces, mk4(0.0f, 0.0f, 0.0f, 0.0f));
    if (tracked) {
      for (int f = 0; f < nFaces; f++) fs[1] += tp_face_record(facePos + 9 * (size_t)f, s->prev.data() + 9 * (size_t)f, s->rec.data() + 3 * (size_t)f) ? 1 : 0;
      faces.pos = facePos; faces.rec = s->rec.data(); faces.first = firstFace; faces.nTracked = nFaces;
    }
    s->prev.assign(facePos, facePos + 9 * (size_t)nFaces);
  }
  if (on) { if (nFaces == 0) s->prev.clear(); s->faceHave = true; s->changed = false; }
  const int prev = s->cur, cur = s->cur ^ 1;
  for (int i = 0; i < 2; i++) { s->col[i].resize(n); s->guide[i].resize(n); s->mom[i].resize(n); }
  std::vector<v4> colA(n), colB(n), side(n);
  std::vector<v4>& guide = s->guide[cur];
  uint64_t cnt[4] = { 0, 0, 0, 0 };
  for (int p = 0; p < n; p++) {
    v4 c, g, sd;
    dn_decode(accum, albedo, normal, depth, hits, nAccumulation, nSamples, demodulate, p, c, g, sd);
    const TpResult r = faces.nTracked > 0
        ? tp_reproject_faces(t, s->col[prev].data(), s->guide[prev].data(), s->mom[prev].data(), motion.data(), faces, p % width, p / width, c, g, primId[p], matId[p])
        : tp_reproject(t, s->col[prev].data(), s->guide[prev].data(), s->mom[prev].data(), motion.data(), p % width, p / width, c, g, primId[p], matId[p]);
    colA[p] = r.col; side[p] = sd;
    s->col[cur][p] = r.hist; guide[p] = g; s->mom[cur][p] = r.mom;
    if (motionOut) { motionOut[2 * (size_t)p] = r.mvx; motionOut[2 * (size_t)p + 1] = r.mvy; }
    if (historyOut) historyOut[p] = r.hist.w;
    if (r.geometry) { cnt[0]++; cnt[1] += r.history ? 1 : 0; cnt[2] += r.history ? 0 : 1; cnt[3] += (uint64_t)r.hist.w; }
    fs[2] += r.movedFace ? 1 : 0;
  }
  atrous_host(k, colA, colB, guide.data(), side.data(), prm->iterations, true, pre, out);
  if (counters) for (int i = 0; i < 4; i++) counters[i] = cnt[i];
  if (faceStats) for (int i = 0; i < 3; i++) faceStats[i] = fs[i];
  s->cur = cur; s->have = true; s->frames++;
  s->width = width; s->height = height; s->nSpheres = nSpheres; s->demodulate = demodulate;
  s->cam = t.cam; s->centres = now;
  return 0;
}

}  // extern "C"
