// api_temporal.hip -- temporal accumulation in front of the denoiser (temporalkernel.hip, pt_temporal.h): the moptix_temporal_* entry
// points and moptix_denoise_temporal of include/moptix.h.  The history lives in the context (api_context.h Temporal); the filter runs
// in the denoiser's scratch and writes the denoiser's output, which moptix_denoise_read / moptix_denoise_bind serve for both entries.
#include <cstring>

#include "api_context.h"
#include "facemotionkernel.h"
#include "temporalkernel.h"

using namespace pt;
using namespace pt::api;

namespace {

v3 to3(const moptix_float3& f) { return mk3(f.x, f.y, f.z); }
TpCamera to_camera(const moptix_cam_params& c) {
  TpCamera t; t.origin = to3(c.origin); t.horizontal = to3(c.horizontal); t.vertical = to3(c.vertical); t.lowerLeft = to3(c.scrLowerLeftCorner);
  return t;
}

}  // namespace

extern "C" {

int moptix_temporal_defaults(moptix_temporal_params* out) {
  if (!out) return fail(nullptr, MOPTIX_ERR_INVALID, "null argument");
  out->alpha = 0.2f; out->alphaMoments = 0.2f; out->depthTolerance = 0.2f; out->normalThreshold = 0.5f;
  out->maxHistory = 32; out->varianceFrames = 4;
  return MOPTIX_OK;
}

int moptix_denoise_temporal(moptix_context c, const moptix_denoise_params* p, const moptix_temporal_params* t, float nAccumulation) {
  // the checks of the arguments themselves come first: they need no context (a NULL one then fails as a null argument)
  if (!p || !t) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  const char* why = dn_bad_params(nAccumulation, p->iterations, p->normalPower, p->demodulate, p->sigmaLuminance, p->sigmaDepth);
  if (!why) why = tp_bad_params(t->alpha, t->alphaMoments, t->depthTolerance, t->normalThreshold, t->maxHistory, t->varianceFrames);
  if (why) return fail(c, MOPTIX_ERR_INVALID, why);
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  size_t px;
  const int rc = denoise_begin(c, false, px);      // the filter runs in the denoiser's scratch, under this call's history guide
  if (rc != MOPTIX_OK) return rc;
  moptix_context_t::Temporal& s = c->tp;
  const int demodulate = p->iterations > 0 ? p->demodulate : 0;
  const int nSpheres = (int)c->spheres.size();
  if (!tp_history_kept(s.have, (int)s.width, (int)s.height, s.nSpheres, s.demodulate, (int)c->params.width, (int)c->params.height, nSpheres, demodulate))
    s.drop();
  for (int i = 0; i < 2; i++) {
    HIPCHK(c, s.col[i].ensure(px), "alloc temporal history");
    HIPCHK(c, s.guide[i].ensure(px), "alloc temporal history");
    HIPCHK(c, s.mom[i].ensure(px), "alloc temporal history");
  }
  HIPCHK(c, s.motionOut.ensure(2 * px), "alloc motion vectors");
  HIPCHK(c, s.historyOut.ensure(px), "alloc history lengths");
  HIPCHK(c, s.counters.ensure(4), "alloc temporal counters");
  HIPCHK(c, s.motion.ensure((size_t)nSpheres), "alloc sphere motion");
  const size_t nGroups = (size_t)((c->params.width + 15) / 16) * ((c->params.height + 15) / 16);
  HIPCHK(c, s.partials.ensure(4 * nGroups), "alloc temporal partials");
  // Per-face motion: the faces are the device copy as it stands now.  Without a usable snapshot (none yet, another face count) every
  // face counts as unmoved and the pass only takes the snapshot; with one, the pass runs only where the faces may have changed since.
  moptix_context_t::Temporal::Faces& fm = s.faces;
  const bool facesOn = c->opt.temporalFaceMotion != 0;
  const size_t nFaces = facesOn && c->dFacePos.p && c->dFacePos.n >= 9 * c->refit.facesOnDevice ? c->refit.facesOnDevice : 0;
  if (!facesOn) fm.have = false;
  const bool tracked = facesOn && fm.have && fm.count == nFaces;
  const bool facePass = facesOn && nFaces > 0 && (!tracked || fm.changed);
  if (facePass) {
    if (fm.prev.p && fm.count != nFaces) fm.release();          // sized for another scene
    HIPCHK(c, fm.prev.ensure(9 * nFaces), "alloc face snapshot");
    HIPCHK(c, fm.rec.ensure(3 * nFaces), "alloc face motion records");
    HIPCHK(c, fm.partials.ensure((size_t)face_motion_blocks(nFaces)), "alloc face motion partials");
    HIPCHK(c, fm.counters.ensure(2), "alloc face motion counters");
  }

  TemporalArgs a;
  memset(&a, 0, sizeof(a));
  denoise_consts(c, p, a.k);
  a.t.width = a.k.width; a.t.height = a.k.height;
  a.t.maxHistory = t->maxHistory; a.t.varianceFrames = t->varianceFrames;
  a.t.alpha = t->alpha; a.t.alphaMoments = t->alphaMoments; a.t.depthTolerance = t->depthTolerance; a.t.normalThreshold = t->normalThreshold;
  a.t.cam = to_camera(c->params.cam);
  a.t.haveHistory = s.have ? 1 : 0;
  if (s.have) {
    const TpCamera prev = to_camera(s.cam);
    tp_solve_consts(prev, a.t);
    a.t.sameCamera = tp_same_camera(prev, a.t.cam) ? 1 : 0;
    a.t.nSpheres = nSpheres;
    s.motionHost.resize((size_t)nSpheres);                    // a member: the call's final synchronise comes before its next change
    for (int i = 0; i < nSpheres; i++) {
      const v3 d = c->spheres[i].center - s.centres[i];
      s.motionHost[i] = mk4(d.x, d.y, d.z, 0.0f);
    }
    if (nSpheres > 0)
      HIPCHK(c, hipMemcpyAsync(s.motion.p, s.motionHost.data(), sizeof(v4) * nSpheres, hipMemcpyHostToDevice, c->stream), "upload sphere motion");
  }
  const moptix_aov_buffers b = aov_ptrs(c);
  a.accum = accum_ptr(c); a.albedo = b.albedo; a.normal = b.normal; a.depth = b.depth; a.hits = b.hits;
  a.primId = b.primId; a.matId = b.matId;
  a.nAccumulation = nAccumulation; a.nSamples = (float)c->aov.samples;
  a.iterations = p->iterations; a.demodulate = demodulate;
  const int prev = s.cur, cur = s.cur ^ 1;
  a.prevCol = s.col[prev].p; a.prevGuide = s.guide[prev].p; a.prevMom = s.mom[prev].p; a.motion = s.motion.p;
  a.histCol = s.col[cur].p; a.histGuide = s.guide[cur].p; a.histMom = s.mom[cur].p;
  a.colA = c->dn.colA.p; a.colB = c->dn.colB.p; a.side = c->dn.side.p;
  a.motionOut = s.motionOut.p; a.historyOut = s.historyOut.p;
  a.partials = reinterpret_cast<uint4*>(s.partials.p);
  a.counters = reinterpret_cast<TemporalCounters*>(s.counters.p);
  a.out = denoise_out(c);
  const uint64_t frames = s.frames;
  s.drop();                                                  // a failure below leaves no half-written history (or face snapshot) behind
  fm.last[0] = fm.last[1] = fm.last[2] = 0;                  // nor the previous call's face counters
  const bool faceMotion = facePass && tracked;               // only then can a record say "moved"
  FaceMotionCounters faceCounts = { 0, 0 };
  if (facePass) {
    FaceMotionArgs f;
    f.now = c->dFacePos.p; f.prev = fm.prev.p; f.rec = fm.rec.p; f.nFaces = (int)nFaces; f.snapshotOnly = tracked ? 0 : 1;
    f.partials = fm.partials.p;
    HIPCHK(c, launch_face_motion(c->stream, f), "launch face motion pass");
  }
  if (faceMotion) { a.faces.pos = c->dFacePos.p; a.faces.rec = fm.rec.p; a.faces.first = nSpheres + (int)c->quads.size(); a.faces.nTracked = (int)nFaces; }
  HIPCHK(c, launch_temporal(c->stream, a), "launch temporal denoiser");
  HIPCHK(c, hipMemcpyAsync(s.last, s.counters.p, sizeof(s.last), hipMemcpyDeviceToHost, c->stream), "read temporal counters");
  if (faceMotion) {
    HIPCHK(c, launch_face_motion_reduce(c->stream, fm.partials.p, face_motion_blocks(nFaces), a.partials, (int)nGroups,
                                        reinterpret_cast<FaceMotionCounters*>(fm.counters.p)), "launch face motion counters");
    HIPCHK(c, hipMemcpyAsync(&faceCounts, fm.counters.p, sizeof(faceCounts), hipMemcpyDeviceToHost, c->stream), "read face motion counters");
  }
  HIPCHK(c, hipStreamSynchronize(c->stream), "temporal denoiser");
  fm.last[0] = tracked ? nFaces : 0; fm.last[1] = faceCounts.movedFaces; fm.last[2] = faceCounts.movedPixels;
  if (facesOn) { fm.have = true; fm.count = nFaces; fm.changed = false; }
  s.cur = cur; s.have = true; s.frames = frames + 1;
  s.width = c->params.width; s.height = c->params.height; s.nSpheres = nSpheres; s.demodulate = demodulate;
  s.cam = c->params.cam;
  s.centres.resize((size_t)nSpheres);
  for (int i = 0; i < nSpheres; i++) s.centres[i] = c->spheres[i].center;
  s.pixels = px;
  c->dn.pixels = px;
  return MOPTIX_OK;
}

int moptix_temporal_reset(moptix_context c) {
  if (!c) return fail(c, MOPTIX_ERR_INVALID, "null context");
  c->tp.drop();
  if (c->tp.faces.prev.p) {                                   // the face snapshot goes with the history
    (void)hipSetDevice(c->device);
    if (!c->poisoned) (void)hipStreamSynchronize(c->stream);
    c->tp.faces.release();
  }
  return MOPTIX_OK;
}

int moptix_temporal_face_info(moptix_context c, moptix_temporal_face_stats* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  const moptix_context_t::Temporal& s = c->tp;
  memset(out, 0, sizeof(*out));
  if (s.pixels == 0) return MOPTIX_OK;
  out->trackedFaces = s.faces.last[0]; out->movedFaces = s.faces.last[1]; out->movedPixels = s.faces.last[2];
  return MOPTIX_OK;
}

int moptix_temporal_info(moptix_context c, moptix_temporal_stats* out) {
  if (!c || !out) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  const moptix_context_t::Temporal& s = c->tp;
  memset(out, 0, sizeof(*out));
  out->frames = s.frames;
  if (s.pixels == 0) return MOPTIX_OK;
  out->geometryPixels = s.last[0]; out->historyPixels = s.last[1]; out->disoccludedPixels = s.last[2];
  out->meanHistory = s.last[0] ? (float)((double)s.last[3] / (double)s.last[0]) : 0.0f;
  return MOPTIX_OK;
}

int moptix_temporal_read(moptix_context c, const moptix_temporal_buffers* dstHost) {
  if (!c || !dstHost) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  const size_t px = (size_t)c->params.width * c->params.height;
  if (c->tp.pixels != px) return fail(c, MOPTIX_ERR_STATE, "no moptix_denoise_temporal call at this frame size");
  const int rc = begin_call(c, false);
  if (rc != MOPTIX_OK) return rc;
  return read_back(c, { { dstHost->motion, c->tp.motionOut.p, sizeof(float) * 2 * px }, { dstHost->history, c->tp.historyOut.p, sizeof(float) * px } },
                   "read motion vectors / history lengths");
}

}  // extern "C"
