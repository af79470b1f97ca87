// api_context.h -- the context record behind moptix_context and the helpers the api_*.hip files share.  Private to them.
#pragma once
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/moptix.h"
#include "lbvh.h"
#include "megakernel.h"
#include "refitkernel.h"
#include "pt_signtopo.h"

namespace pt { struct WindingNode; }      // pt_winding.h (api_winding.hip is the only file that needs its size)
struct ncclComm;      // RCCL's communicator (api_comm.hip is the only file that sees RCCL's declarations)

namespace pt { namespace api {

template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  hipError_t ensure(size_t count) {
    if (count <= n && p) return hipSuccess;
    if (p) { (void)hipFree(p); p = nullptr; n = 0; }
    hipError_t e = hipMalloc((void**)&p, sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) n = count ? count : 1;
    return e;
  }
  hipError_t upload(const std::vector<T>& v, hipStream_t s) {
    hipError_t e = ensure(v.size());
    if (e != hipSuccess || v.empty()) return e;
    return hipMemcpyAsync(p, v.data(), sizeof(T) * v.size(), hipMemcpyHostToDevice, s);
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// Unit ids in descending order of their keys, ties in id order: the depth history of the beauty launches (keys: the cost buffer the trace
// kernels write, LaunchArgs::tileCost; units: pixels or 8x8 tiles) and the adaptive passes' list (keys: k_ad_mask's, one per pixel slot).
// Defined in api_render.hip, beside the one instantiation of rocprim's sort.
struct OrderList {
  long long units = -1;              // units the list holds (-1 = none: the next ensure() starts it afresh)
  DevBuf<unsigned int> keys, keysSorted; DevBuf<int> order, iota; DevBuf<uint8_t> sortTmp;
  // n units: no-op when the list holds n, else buffers, iota, zero keys and the sort's scratch; synchronises the stream
  hipError_t ensure(long long n, hipStream_t stream);
  hipError_t sort(hipStream_t stream);      // keys -> order (stable radix sort, descending), asynchronously
  void forget() { units = -1; }
  void release() { keys.release(); keysSorted.release(); order.release(); iota.release(); sortTmp.release(); units = -1; }
};

// moptix_set_option / moptix_get_option (api_core.hip kOptions: names, accepted values, what a change invalidates)
struct Options {
  int exitThreshold = 16, leafSize = 4, blocksPerCU = 3;
  int kernelVariant = -1;         // -1 = the library's own choice per launch (api_render.hip plan_launch), else the caller's: 0, 3 or 4
  int tileMajor = 3;              // all samples of a pixel back to back, pixels with the deepest paths of earlier launches first
  int starveLanes = 16, sampleBufMB = 16384, leafThreshold = 16, swapLanes = 32;
  int watchdogMs = 600000;
  int nodeFormat = 0;             // the node record the packet kernel fetches (pt_types.h): 64, 128, or 0 = whichever costs this scene less (choose_node_format)
  int fastShading = 0;
  int builder = 1;
  int analyticQueue = -1;         // -1 = by primitive count
  int autoPacket = 1;
  int commBlocking = 0;           // 1 = plain ncclCommInitRank even where a non-blocking communicator is available
  int commTimeoutMs = 120000;     // deadline of a collective's completion (comm_wait); the first collective of a communicator also sets its links up
  int shadowRule = 1;             // 1 = a shadow ray is decided by its nearest any-hit surface (default), 0 = SURVEY A2's order-independent rule
  int slotsInUse = -1;            // -1 = chosen per launch from its size
  int drainBelow = 64;            // a workgroup of the packet kernel with this many paths left hands them to the drain kernel (0 = off)
  int auxDepth = 16;              // variant 4: depth from which a path's shadow rays get slots of their own (0 = off)
  int specialize = 1;             // variant 4: a scene whose tables rule out every FEAT_* program (pt_types.h) runs the build without them (0 = always the general one)
  int queryBlocksPerCU = 32;      // ray queries (querykernel.hip): the grid's cap in workgroups per CU; beyond it lanes loop over rays
  int temporalFaceMotion = 0;     // 1 = moptix_denoise_temporal reprojects moved triangles through their own motion (api_temporal.hip)
  int radianceBufferMB = 256;     // radiance queries (radiancekernel.hip): the per-sample scratch a launch may use; a longer call runs in passes
};

}}  // namespace pt::api

struct moptix_context_t {
  template <class T> using DevBuf = pt::api::DevBuf<T>;

  // ---- device, stream, error, frame (api_core.hip) ----
  int device = 0;
  int numCUs = 256;
  hipStream_t stream = nullptr; bool ownStream = false;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  std::string err;
  bool poisoned = false;             // a dead collective's kernels are still on the stream (comm_teardown): every call fails from here on
  moptix_params params{}; bool haveParams = false;
  int rank = 0, nRanks = 1;          // moptix_set_partition
  pt::api::Options opt;

  // ---- scene (api_core.hip): host staging (copied from the caller, as OptiX copies on setUserData / map+memcpy), its device copy, the tree ----
  std::vector<pt::DevMaterial> mats;
  std::vector<pt::DevSphere> spheres; std::vector<int> sphereMat;
  std::vector<pt::DevQuad> quads;
  std::vector<pt::DevLight> lights;
  std::vector<float> facePos, faceNrm; std::vector<int> faceHasNrm, faceMat;
  std::vector<pt::TriUV> faceUV; bool anyUV = false;
  struct HostTexture { int width, height; std::vector<float> rgba; };
  std::vector<HostTexture> textures;
  bool sceneDirty = true, accelBuilt = false;
  DevBuf<pt::DevMaterial> dMats; DevBuf<pt::DevSphere> dSpheres; DevBuf<int> dSphereMat; DevBuf<pt::DevQuad> dQuads; DevBuf<pt::DevLight> dLights;
  DevBuf<float> dFacePos, dFaceNrm; DevBuf<int> dFaceHasNrm, dFaceMat;
  DevBuf<pt::TriUV> dFaceUV; DevBuf<float> dTexels; DevBuf<pt::DevTexture> dTextures;
  pt::LbvhResult bvh;
  double glassFaceShare = 0.0;       // triangles whose material is glass (no next-event estimation at their hits), set by build_accel
  void release_scene() {
    dMats.release(); dSpheres.release(); dSphereMat.release(); dQuads.release(); dLights.release();
    dFacePos.release(); dFaceNrm.release(); dFaceHasNrm.release(); dFaceMat.release();
    dFaceUV.release(); dTexels.release(); dTextures.release();
    pt::lbvh_free(&bvh);
  }

  // ---- accumulation buffer and 8-bit resolve (api_core.hip) ----
  DevBuf<float> dAccum; float* accumBound = nullptr; size_t accumPixels = 0;
  bool accumPlain = false;           // moptix_launch / render* have added to the accumulation buffer since its last clear (api_adaptive.hip)
  DevBuf<uint8_t> dRgb8;

  // ---- beauty launches (api_render.hip) ----
  int nodeFormatUsed = 128;          // the verdict for this build (get_option "node_format_used")
  bool formatDecided = false;
  unsigned long long probeCounts[4] = { 0, 0, 0, 0 };     // node steps, triangle tests of the probe rays under Node128; the same under Node64
  int lastVariant = -1;              // what the last render ran (get_option "kernel_variant_used")
  int lastFeatures = pt::FEAT_ALL;   // the FEAT_* mask compiled into that render's trace kernel (get_option "kernel_features_used")
  int lastSlim = 0;                  // 1: that kernel was the packet kernel's slim build (get_option "kernel_slim_used")
  int countedSpanUs = -1, countedTailUs = -1;   // last counted launch: first wave in -> last wave out, and the part of it after the last work item was handed out
  double kernelMs = 0.0, reduceMs = 0.0; uint64_t nLaunches = 0;
  bool asyncPending = false;
  std::vector<int> seedStaging;
  // Pinned staging of a batch's small uploads, the work header and the seeds (api_render.hip launch_staging): the copies from it are
  // asynchronous, so moptix_render_async does not wait for the stream; the event behind the last copy says when it may be written again.
  int* launchStaging = nullptr; size_t launchStagingInts = 0; hipEvent_t launchStaged = nullptr;
  DevBuf<int> dSeeds; DevBuf<int> dWork; DevBuf<unsigned long long> dCounters; DevBuf<int> dOverflow;
  DevBuf<uint8_t> dPoolCold; DevBuf<float> dSampleBuf;
  void release_render() {
    dSeeds.release(); dWork.release(); dCounters.release(); dOverflow.release(); dPoolCold.release(); dSampleBuf.release();
    tiles.release();
    if (launchStaging) (void)hipHostFree(launchStaging);
    if (launchStaged) (void)hipEventDestroy(launchStaged);
    launchStaging = nullptr; launchStagingInts = 0; launchStaged = nullptr;
  }
  // which units (pixels or 8x8 tiles) had the deepest paths in earlier launches: they are handed out first (LaunchArgs::tileOrder);
  // forgotten by a new scene, partition or granularity
  pt::api::OrderList tiles;

  // ---- multi-GPU, one process per GPU (api_comm.hip): RCCL communicator of this rank + staging for the tile gather ----
  struct Comm {
    ncclComm* handle = nullptr; int rank = 0, ranks = 1;
    bool nonBlocking = false;        // the communicator was made with config.blocking = 0 (calls may return ncclInProgress: comm_settle)
    DevBuf<float> tileSend, tileRecv;
  } comm;                            // released by pt::api::comm_release

  // ---- first-hit AOVs (api_aov.hip): allocated at the first AOV call; a bound member (moptix_aov_bind) replaces the own buffer ----
  struct Aov {
    DevBuf<float> albedo, normal, depth, hits; DevBuf<int> primId, matId;
    moptix_aov_buffers bound{};
    size_t pixels = 0;               // frame size the AOV buffers hold (0 = to be (re)allocated and cleared at the next AOV call)
    uint64_t samples = 0;            // seeds added since the clear
    DevBuf<int> seeds, work, overflow;
    void frame_resized() { pixels = 0; samples = 0; }      // the AOVs are reallocated and cleared at the next AOV call
    void release() {
      albedo.release(); normal.release(); depth.release(); hits.release(); primId.release(); matId.release();
      seeds.release(); work.release(); overflow.release();
    }
  } aov;

  // ---- denoiser (api_denoise.hip): scratch and output allocated at the first call, freed by a frame-size change; a bound output
  // (moptix_denoise_bind) replaces the own one ----
  struct Denoise {
    DevBuf<pt::v4> colA, colB, guide, side; DevBuf<float> out;
    float* bound = nullptr;
    size_t pixels = 0;               // frame size of the last denoise call (0: none since the last frame-size change)
    void release() { colA.release(); colB.release(); guide.release(); side.release(); out.release(); pixels = 0; }
  } dn;

  // ---- temporal accumulation (api_temporal.hip): the history of moptix_denoise_temporal, two sets that swap roles per call; allocated
  // at the first call, freed by a frame-size change.  The filter itself runs in the denoiser's scratch and writes the denoiser's output ----
  struct Temporal {
    DevBuf<pt::v4> col[2], guide[2], mom[2];   // {I_acc, h}, {N, Z}, {m1, m2, matId, -} (csrc/pt_temporal.h)
    DevBuf<pt::v4> motion;                     // per sphere: centre now - centre at the previous call
    DevBuf<float> motionOut, historyOut;       // last call's motion vectors (W*H*2) and history lengths (W*H)
    DevBuf<unsigned long long> counters;       // TemporalCounters
    DevBuf<unsigned int> partials;             // four words per 16x16 workgroup of the reproject kernel
    std::vector<pt::v4> motionHost;            // staging of `motion`: outlives the asynchronous upload
    int cur = 0;                               // the set the last call wrote
    bool have = false;                         // a history to reproject from (false: the next call is a first frame)
    uint32_t width = 0, height = 0; int nSpheres = 0, demodulate = 0;     // what the history was made with
    moptix_cam_params cam{}; std::vector<pt::v3> centres;                 // snapshot at the end of the last call
    uint64_t frames = 0;                       // calls since the last drop
    size_t pixels = 0;                         // frame size of the last call's motion vectors / history lengths (0: none)
    unsigned long long last[4] = { 0, 0, 0, 0 };
    // Per-face motion (option "temporal_face_motion", facemotionkernel.hip).  The snapshot holds the device copy of the faces as the
    // last call with the option on saw it; it goes with the history, with the scene, with a different face count and with the option.
    struct Faces {
      DevBuf<float> prev;                      // the snapshot: 9 floats per face
      DevBuf<pt::v4> rec;                      // three displacement records per face (pt_temporal.h TpFaces)
      DevBuf<unsigned int> partials;           // moved faces per workgroup of the face pass
      DevBuf<unsigned long long> counters;     // FaceMotionCounters
      bool have = false; size_t count = 0;     // a snapshot exists, of so many faces
      bool changed = true;                     // the faces may differ from the snapshot (moptix_update_faces*, moptix_build_accel, moptix_clear_scene)
      unsigned long long last[3] = { 0, 0, 0 };       // moptix_temporal_face_info: tracked faces, moved faces, moved pixels of the last call
      void release() { prev.release(); rec.release(); partials.release(); counters.release(); have = false; count = 0; }
    } faces;
    void drop() { have = false; frames = 0; faces.have = false; }
    void release() {
      for (int i = 0; i < 2; i++) { col[i].release(); guide[i].release(); mom[i].release(); }
      motion.release(); motionOut.release(); historyOut.release(); counters.release(); partials.release();
      faces.release();
      drop(); pixels = 0;
    }
  } tp;

  // ---- adaptive sampling (api_adaptive.hip): per-pixel counts, luminance moments, the sticky converged flags and the order list of
  // the adaptive passes; allocated and zeroed at the first adaptive call, dropped by whatever changes the accumulation buffer behind
  // its back (frame-size change, moptix_accum_clear, moptix_accum_bind, a clearing moptix_resolve_rgb8) ----
  struct Adaptive {
    DevBuf<uint32_t> count; DevBuf<float> moments, error; DevBuf<uint8_t> converged;
    pt::api::OrderList order;                  // the pixel slots, active ones first
    DevBuf<unsigned int> partials, totals;     // four words per 16x16 workgroup of the mask kernel; AdaptiveTotals
    DevBuf<float> mean;                        // staging of moptix_adaptive_mean (allocated at its first call)
    size_t pixels = 0;               // frame size the state holds (0 = to be (re)allocated and zeroed at the next adaptive call)
    bool have = false;               // samples added since the clear: count describes the accumulation buffer
    void drop() { pixels = 0; have = false; }
    void release() {
      count.release(); moments.release(); error.release(); converged.release();
      order.release(); partials.release(); totals.release(); mean.release();
      drop();
    }
  } ad;

  // ---- ray queries (api_query.hip): the stack overflow area of the query kernel, allocated at the first query after a build and
  // dropped with the tree it was sized for (moptix_clear_scene, moptix_build_accel); the staging of the host-pointer entry point.  The
  // multi-hit queries use all three as they are (out: the records, the counts behind them) ----
  struct Query {
    DevBuf<int> overflow;
    DevBuf<float> rays; DevBuf<uint8_t> out;
    void drop() { overflow.release(); }
    void release() { drop(); rays.release(); out.release(); }
  } query;

  // ---- radiance queries (api_radiance.hip): the per-sample scratch, the work counter and the seeds' device copy, allocated at first use
  // and kept; the stack overflow area of the radiance kernel, allocated at the first radiance query after a build and dropped with the tree
  // it was sized for, where the ray queries' is; the staging of the host-pointer entry point ----
  struct Radiance {
    DevBuf<int> overflow;
    DevBuf<float> scratch; DevBuf<int> work, seeds;
    int* seedStaging = nullptr; size_t seedStagingN = 0;      // pinned: the seeds' upload is asynchronous
    hipEvent_t seedsUploaded = nullptr;                       // recorded behind that upload: the staging is free again once it has passed
    DevBuf<float> rays, out; DevBuf<uint32_t> states;
    void drop() { overflow.release(); }
    void release() {
      drop(); scratch.release(); work.release(); seeds.release(); rays.release(); out.release(); states.release();
      if (seedStaging) (void)hipHostFree(seedStaging);
      if (seedsUploaded) (void)hipEventDestroy(seedsUploaded);
      seedStaging = nullptr; seedStagingN = 0; seedsUploaded = nullptr;
    }
  } radiance;

  // ---- point queries (api_point.hip): the stack overflow area of the point kernel, its own (eight bytes an entry: reference + box
  // distance), allocated at the first point query after a build and dropped with the tree it was sized for, where the ray queries' is;
  // the staging of the host-pointer entry point.  The K-nearest queries use all three as they are (out: the records, the counts behind
  // them) ----
  struct Point {
    DevBuf<unsigned long long> overflow;
    DevBuf<float> points; DevBuf<uint8_t> out;
    void drop() { overflow.release(); }
    void release() { drop(); points.release(); out.release(); }
  } point;

  // ---- box queries (api_box.hip): the stack overflow area of the box kernel, its own (four bytes an entry: a reference), allocated at
  // the first box query after a build, kept across refits and dropped with the tree it was sized for, where the ray queries' is; the
  // staging of the host-pointer entry points (boxes, offsets, prims; out: the int32 results or counts) ----
  struct Box {
    DevBuf<int> overflow;
    DevBuf<float> boxes; DevBuf<long long> offsets; DevBuf<int> prims, out;
    void drop() { overflow.release(); }
    void release() { drop(); boxes.release(); offsets.release(); prims.release(); out.release(); }
  } box;

  // ---- sweep queries (api_sweep.hip): the stack overflow area of the sweep kernel, its own (eight bytes an entry: reference + entry
  // time), allocated at the first sweep query after a build, kept across refits and dropped with the tree it was sized for, where the
  // ray queries' is; the staging of the host-pointer entry point ----
  struct Sweep {
    DevBuf<unsigned long long> overflow;
    DevBuf<float> sweeps; DevBuf<uint8_t> out;
    void drop() { overflow.release(); }
    void release() { drop(); sweeps.release(); out.release(); }
  } sweep;

  // ---- segment queries (api_segment.hip): the stack overflow area of the segment kernel, its own (eight bytes an entry: reference +
  // box distance), allocated at the first segment query after a build, kept across refits and dropped with the tree it was sized for,
  // where the ray queries' is; the staging of the host-pointer entry point ----
  struct Segment {
    DevBuf<unsigned long long> overflow;
    DevBuf<float> segments; DevBuf<uint8_t> out;
    void drop() { overflow.release(); }
    void release() { drop(); segments.release(); out.release(); }
  } segment;

  // ---- oriented box queries (api_obb.hip): the stack overflow area of the oriented box kernel, its own (four bytes an entry: a
  // reference), allocated at the first such query after a build, kept across refits and dropped with the tree it was sized for, where the
  // box queries' is; the staging of the host-pointer entry points (obbs, offsets, prims; out: the int32 results or counts) ----
  struct ObbQuery {
    DevBuf<int> overflow;
    DevBuf<float> obbs; DevBuf<long long> offsets; DevBuf<int> prims, out;
    void drop() { overflow.release(); }
    void release() { drop(); obbs.release(); offsets.release(); prims.release(); out.release(); }
  } obb;

  // ---- triangle queries (api_tri.hip): the stack overflow area of the triangle query kernel, its own (four bytes an entry: a reference),
  // allocated at the first such query after a build, kept across refits and dropped with the tree it was sized for, where the box
  // queries' is; the staging of the host-pointer entry points (tris, offsets, prims; out: the int32 results or counts) ----
  struct TriQuery {
    DevBuf<int> overflow;
    DevBuf<float> tris; DevBuf<long long> offsets; DevBuf<int> prims, out;
    void drop() { overflow.release(); }
    void release() { drop(); tris.release(); offsets.release(); prims.release(); out.release(); }
  } tri;

  // ---- frustum queries (api_frustum.hip): the stack overflow area of the frustum kernel, its own (four bytes an entry: a reference),
  // allocated at the first such query after a build, kept across refits and dropped with the tree it was sized for, where the box
  // queries' is; the staging of the host-pointer entry points (frusta, offsets, prims; out: the int32 results or counts) ----
  struct FrustumQuery {
    DevBuf<int> overflow;
    DevBuf<float> frusta; DevBuf<long long> offsets; DevBuf<int> prims, out;
    void drop() { overflow.release(); }
    void release() { drop(); frusta.release(); offsets.release(); prims.release(); out.release(); }
  } frustum;

  // ---- winding-number queries (api_winding.hip): nothing of this exists in a context that never asks for a winding number.  The stack
  // overflow area of the winding kernel, its own (four bytes an entry), and the table of cluster moments (128 bytes per node) are
  // allocated at the first such query after a build and dropped with the tree they were sized for, where the box queries' area is.
  // stale: the faces may have moved or the boxes changed since the table was computed (set by moptix_update_faces*, moptix_refit_accel
  // and moptix_build_accel); the next winding query enqueues the moments pass in front of its kernel.  The staging of the host-pointer
  // entry point ----
  struct Winding {
    DevBuf<int> overflow;
    DevBuf<pt::WindingNode> table; bool stale = true;
    uint32_t tableBuilds = 0;          // moments passes enqueued by this context so far (moptix_get_winding_info)
    DevBuf<float> points, out;
    void drop() { overflow.release(); table.release(); stale = true; }
    void release() { drop(); points.release(); out.release(); }
  } winding;

  // ---- signed point queries (api_sign.hip) ----
  // The topology belongs to one set of uploaded faces: taken on the host at the first signed query or moptix_get_sign_info, kept across
  // moptix_update_faces*, moptix_refit_accel and moptix_build_accel, dropped by moptix_clear_scene, moptix_add_mesh and destroy.  Its
  // device copy and the table are allocated at the first signed query and kept with it.  stale: the faces may have moved since the table
  // was computed (set by the three calls that keep the topology); the next signed query enqueues the table build in front of its kernel.
  struct Sign {
    bool have = false, uploaded = false, stale = true;
    pt::SignTopology topo;
    uint32_t tableBuilds = 0;
    DevBuf<int> faceIds, vertexStart, vertexCorner, edgeStart, edgeFace;
    DevBuf<pt::SignFace> faces; DevBuf<pt::v4> vertexN, edgeN; DevBuf<pt::SignRecord> table;
    void release() {
      faceIds.release(); vertexStart.release(); vertexCorner.release(); edgeStart.release(); edgeFace.release();
      faces.release(); vertexN.release(); edgeN.release(); table.release();
      topo = pt::SignTopology(); have = false; uploaded = false; stale = true; tableBuilds = 0;
    }
  } sign;

  // ---- mesh updates and refit (api_refit.hip) ----
  // facesDirty: positions changed since the tree was built or refitted (check_ready refuses to trace); hostStale: the device copy of the
  // faces is ahead of the host staging (moptix_update_faces_device; moptix_build_accel fetches it back first); facesOnDevice: how many
  // faces moptix_build_accel uploaded -- the first so many of the staging, which moptix_add_mesh may have grown since.
  // The refit plan belongs to one built tree: the levels of the emitted four-wide tree, the raw boxes by sorted slot and the scratch of the
  // passes.  Made at the first refit after a build, dropped by moptix_build_accel, moptix_clear_scene and destroy.
  struct Refit {
    bool facesDirty = false, hostStale = false;
    size_t facesOnDevice = 0;
    bool planned = false;
    DevBuf<int> levelOrder; std::vector<int> levelFirst;      // pt_refit.h refit_plan_levels
    DevBuf<pt::RefitBox> raw; DevBuf<uint32_t> sceneBox; DevBuf<double> partials; DevBuf<pt::RefitCost> cost; DevBuf<int> bad;
    struct Pinned { pt::RefitCost cost; int bad; }* pinned = nullptr;      // where the folded cost and the Node64 verdict come back
    hipEvent_t e0 = nullptr, e1 = nullptr;
    moptix_refit_info info{};
    void drop() {
      levelOrder.release(); levelFirst.clear(); raw.release(); sceneBox.release(); partials.release(); cost.release(); bad.release();
      if (pinned) (void)hipHostFree(pinned);
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
      pinned = nullptr; e0 = nullptr; e1 = nullptr; planned = false; info = moptix_refit_info{};
    }
  } refit;
};

namespace pt {
struct DenoiseConsts;      // pt_denoise.h
namespace api {

// the error text goes to the context, or (no context: moptix_create, moptix_comm_unique_id) to the library's own
int fail(moptix_context c, int code, const std::string& msg);
int hipFail(moptix_context c, hipError_t e, const char* what);
#define HIPCHK(c, x, what) do { hipError_t e_ = (x); if (e_ != hipSuccess) return pt::api::hipFail((c), e_, (what)); } while (0)

int check_ready(moptix_context c);                   // params set, tree built and fitted to the faces, stream alive
int fetch_faces(moptix_context c);                   // api_refit.hip: the host staging catches up with device-side face updates
// api_sign.hip, for api_point.hip: the sign table as the faces are now, for a kernel enqueued after this call (the topology, its upload and
// the table build are enqueued on the context's stream where they are missing or stale); null in a scene without triangles
int sign_table_for_query(moptix_context c, const SignRecord*& table);
void sign_release(moptix_context c);                 // the topology goes (a query in flight finishes first)
void winding_release(moptix_context c);              // api_winding.hip: the moments table and the overflow area go (a query in flight finishes first)
int refit_plan(moptix_context c);                    // api_refit.hip: the refit's plan of the built tree (c->refit.levelOrder, levelFirst), made where it is missing
float* accum_ptr(moptix_context c);
int ensure_accum(moptix_context c);
// What a call that uses the device starts with: hipSetDevice, the batch in flight finishes (moptix_sync: timed, watchdog flag read) and,
// withAccum, the accumulation buffer exists at this frame size.
int begin_call(moptix_context c, bool withAccum);
// Copies every entry with a host destination from its device buffer, then synchronises the stream.
struct ReadBack { void* dst; const void* src; size_t bytes; };
int read_back(moptix_context c, std::initializer_list<ReadBack> copies, const char* what);
void fill_view(moptix_context c, SceneView& v);
// The FEAT_* programs (pt_types.h) the scene's tables can reach, as they are now: materials, lights and textures change between launches.
int scene_features(moptix_context c);
// The scene as a query sees it (api_query.hip, api_radiance.hip, api_point.hip): the 64-byte nodes wherever the tree has them and option
// "node_format" does not say 128 -- the node-format verdict of the render path is not consulted.  Returns the launch's cap of workgroups.
int fill_query_view(moptix_context c, SceneView& v);
moptix_aov_buffers aov_ptrs(moptix_context c);       // api_aov.hip: bound or own, member by member
void comm_release(moptix_context c);                 // api_comm.hip: destroys the communicator, frees the staging
// api_denoise.hip, for moptix_denoise and moptix_denoise_temporal alike: the context is usable and has AOV samples, begin_call, the
// scratch (guide: only the spatial entry's own; the temporal one filters under its history's) and the own output unless one is bound
int denoise_begin(moptix_context c, bool ownGuide, size_t& px);
void denoise_consts(moptix_context c, const moptix_denoise_params* p, DenoiseConsts& k);
inline float* denoise_out(moptix_context c) { return c->dn.bound ? c->dn.bound : c->dn.out.p; }

// ---- the launch plan (api_render.hip): what one batch of launches will run, decided from the context, the batch size and whether it counts ----
struct LaunchPlan {
  const TraceKernel* kernel;      // kPacketKernel, kQueueKernel, kLeanQueueKernel, or null = the per-lane megakernel (launch_megakernel)
  int variant;                    // the same as get_option "kernel_variant_used" reports it: 4, 3, 0
  PacketBuild build;              // variant 4: the build of the packet kernel the launches run (megakernel.h packet_build); General for every other kernel
  int nItems, tilesX;             // pixel slots of this rank (local tiles * 64); 8x8 tiles per row of the frame
  int nBlocks;
  long long perPass;              // launches per pass, before the out-of-memory halving of the per-sample buffer
  int slotsInUse, auxDepth, drainBelow, ovfDepth;
  int tileMajor, unitShift; long long historyUnits;
  size_t poolBytes, overflowInts, workInts;      // path-slot records; stack overflow area; work counter + watchdog flag + drain list
};
// A prepared batch: the plan, the kernel arguments with every buffer the plan asks for in place, and the seeds one pass may take.
struct RenderLaunch {
  LaunchPlan p; LaunchArgs a;
  long long perPass;              // the plan's, after the out-of-memory halving
  int handoutDivisor, handoutSeeds;      // what the hand-out constants in front of the work counter were made for (megakernel.h handout_consts)
  int* seedStaging;               // pinned room for the batch's nSeeds seeds, free to be written: who copies from it records c->launchStaged behind the copy
  bool counted, fast;
};
// What an adaptive pass hands to launch_pass instead of the defaults: its own order list (the first nWork / nSeeds entries are the
// pixel slots to render) and its own reduction of the per-sample buffer.
struct PassOverride {
  const int* order; int nWork;
  hipError_t (*reduce)(hipStream_t stream, const LaunchArgs& a, void* user); void* user;
};
// byPixelSlots: the plan of an adaptive pass -- hand-out by pixel ("tile_major" 3) through a kernel that keeps its paths in slots, whatever
// the options "tile_major", "kernel_variant" and "analytic_queue" say.
// prepare_launch: node format, plan, buffers, work header, depth history; r.p.nItems == 0 -> nothing to render.  The seeds are the
// caller's to upload (c->dSeeds).
int prepare_launch(moptix_context c, int32_t nSeeds, bool counted, bool byPixelSlots, RenderLaunch& r);
// One pass of n seeds from dSeeds: [order list sorted] trace kernel (+ drain kernel) and the reduction, between the context's events;
// asynchronous (moptix_sync times it and reads the watchdog flag).
int launch_pass(moptix_context c, RenderLaunch& r, const int* dSeeds, int n, const PassOverride* over);

}}  // namespace pt::api
