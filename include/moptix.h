/*
 * moptix.h -- C ABI of the MI355X-native device layer that replaces the OptiX 5
 * host API + rtTrace/acceleration + .cu programs on the MinimalOptiX render path.
 *
 * The reference has no FFI of its own: the path sits behind the OptiX C++ host
 * API (optixpp) as called by class MinimalOptiX.  Each entry point below names
 * the reference call site(s) it replaces (paths relative to
 * /root/reference/MinimalOptiX/).  Plain pointers and sizes only; host memory
 * passed in is copied (as OptiX does on setUserData/map+memcpy); no exceptions
 * cross this boundary -- every function returns MOPTIX_OK (0) or a negative
 * error code and moptix_last_error() gives the text.
 *
 * Built as minimaloptix_amd/lib/libmoptix.so (hipcc --offload-arch=gfx950).
 * There is NO CPU fallback behind this ABI: without a gfx950 device every
 * compute entry point fails with MOPTIX_ERR_NO_DEVICE.
 */
#ifndef MOPTIX_H
#define MOPTIX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOPTIX_OK                 0
#define MOPTIX_ERR_INVALID       -1   /* bad argument / bad handle                 */
#define MOPTIX_ERR_NO_DEVICE     -2   /* no HIP device / not gfx950                 */
#define MOPTIX_ERR_HIP           -3   /* HIP runtime error (text in last_error)     */
#define MOPTIX_ERR_STATE         -4   /* call order (e.g. launch before build_accel)*/
#define MOPTIX_ERR_LIMIT         -5   /* scene exceeds a compiled limit             */
#define MOPTIX_ERR_COMM          -6   /* a collective did not complete (peer missing / communicator error); the communicator was aborted */

typedef struct moptix_context_t* moptix_context;

/* ---- records crossing host<->device (Structures.h) ----------------------- */
typedef struct moptix_float3 { float x, y, z; } moptix_float3;
typedef struct moptix_float4 { float x, y, z, w; } moptix_float4;

/* Structures.h:12-20 CamParams */
typedef struct moptix_cam_params {
  moptix_float3 origin, horizontal, vertical, scrLowerLeftCorner, u, v;
  float lensRadius;
} moptix_cam_params;

/* Structures.h:22-26 SphereParams (velocity is host-side animation state, unused on device) */
typedef struct moptix_sphere_params { float radius; moptix_float3 center; moptix_float3 velocity; } moptix_sphere_params;

/* Structures.h:28-33 QuadParams, as produced by setQuadParams (utils_host.cpp:67-75).
 * Unpadded here; the reference's float4 alignment padding is not part of the ABI. */
typedef struct moptix_quad_params { moptix_float4 plane; moptix_float3 v1, v2, anchor; } moptix_quad_params;

/* which closest-hit program the material carries (Material.cu:28,49,72,118,238) */
enum { MOPTIX_MAT_LAMBERTIAN = 0, MOPTIX_MAT_METAL = 1, MOPTIX_MAT_GLASS = 2, MOPTIX_MAT_DISNEY = 3, MOPTIX_MAT_LIGHT = 4 };
enum { MOPTIX_BRDF_NORMAL = 0, MOPTIX_BRDF_GLASS = 1 };   /* Structures.h:49 BrdfType   */
enum { MOPTIX_LIGHT_SPHERE = 0, MOPTIX_LIGHT_QUAD = 1 };  /* Structures.h:68 LightShape */

/* Structures.h:51-66 DisneyParams */
typedef struct moptix_disney_params {
  int32_t albedoID;              /* 0 = RT_TEXTURE_ID_NULL, else an id from moptix_add_texture */
  moptix_float3 color, emission;
  float metallic, subsurface, specular, roughness, specularTint, anisotropic;
  float sheen, sheenTint, clearcoat, clearcoatGloss;
  int32_t brdfType;
} moptix_disney_params;

/* Structures.h:70-80 LightParams */
typedef struct moptix_light_params {
  moptix_float3 position, normal, emission, u, v;
  float area, radius;
  int32_t shape;
} moptix_light_params;

/* One material = createMaterial + setClosestHitProgram(0, kind) [+ setAnyHitProgram(1,
 * disneyAnyHit) for MOPTIX_MAT_DISNEY] + setUserData of the matching params
 * (Structures.h:35-47 Lambertian/Metal/Glass, :51 Disney, :70 Light.emission). */
typedef struct moptix_material {
  int32_t kind;
  moptix_float3 albedo;          /* LambertianParams / MetalParams / GlassParams .albedo */
  float fuzz;                    /* MetalParams.fuzz   */
  float refIdx;                  /* GlassParams.refIdx */
  moptix_float3 emission;        /* light material: LightParams.emission */
  moptix_disney_params disney;   /* MOPTIX_MAT_DISNEY */
} moptix_material;

/* Context variables (MinimalOptiX.cpp:136-151), miss bgColor (:165...), raygen
 * camParams (:256...) and the launch size (:546). */
typedef struct moptix_params {
  uint32_t width, height;        /* fixedWidth/fixedHeight, MinimalOptiX.h:82-83 */
  uint32_t rayMaxDepth;          /* 256   MinimalOptiX.h:85 */
  float rayMinIntensity;         /* 0.001 MinimalOptiX.h:88 */
  float rayEpsilonT;             /* 0.001 MinimalOptiX.h:89 */
  moptix_float3 bgColor;         /* staticMiss bgColor, miss.cu:7 */
  moptix_cam_params cam;
} moptix_params;

/* Counters of a counting launch (moptix_render_counted): the algorithmic-byte
 * model of SURVEY 8(d) is evaluated from these. */
typedef struct moptix_stats {
  uint64_t samples;              /* camera samples traced                                 */
  uint64_t primaryRays, bounceRays, shadowRays;
  uint64_t nodeFetches;          /* four-child BVH nodes fetched: 64-byte records where get_option "node_format_used" says 64
                                    (variant 4 on scenes whose paths favour the quantised form), else 128-byte ones */
  uint64_t triTests;             /* 48-byte triangle records tested                       */
  uint64_t closestHits;          /* closest-hit shading fetches                           */
  uint64_t lightLoads;           /* LightParams records read for NEE                      */
  uint64_t analyticTests;        /* sphere/quad records tested (brute-force lists)        */
  uint64_t traversalSteps;       /* wave-level loop iterations (x64 lanes = lane slots)   */
  uint64_t activeLaneSteps;      /* lanes doing useful work summed over those iterations  */
  uint64_t shadeBatches;         /* shading / regeneration batches run (queue kernels)     */
  uint64_t shadeBatchLanes;      /* slots processed by those batches                       */
} moptix_stats;

typedef struct moptix_accel_info {
  uint32_t nTriangles, nNodes, maxLeafSize, treeDepth;
  float buildMs;                 /* wall time of the last acceleration build between two HIP events on the launch stream: its kernels plus the
                                    host round trips between them (the binned-SAH builder reads one node count per level back) */
  uint64_t nodeBytes, triBytes;  /* nodeBytes: both forms of the nodes, nNodes x (128 + 64) */
} moptix_accel_info;

/* ---- lifecycle: Context::create()/setRayTypeCount/setEntryPointCount/setStackSize
 *      (MinimalOptiX.cpp:131-134) --------------------------------------------- */
int moptix_create(moptix_context* out, int device);
int moptix_destroy(moptix_context ctx);
const char* moptix_last_error(moptix_context ctx);           /* ctx may be NULL: last global error */
const char* moptix_version(void);
/* run every launch on this hipStream_t (default: a stream the context owns) */
int moptix_set_stream(moptix_context ctx, void* hipStream);

/* ---- parameters: context[...]->set* (MinimalOptiX.cpp:136-151,165,256) ---- */
int moptix_set_params(moptix_context ctx, const moptix_params* p);

/* ---- scene upload (MinimalOptiX.cpp:168-249, 362-537, 780-843) ------------ */
int moptix_clear_scene(moptix_context ctx);
/* createTextureSampler + createBuffer(RT_BUFFER_INPUT, RT_FORMAT_FLOAT4, w, h) + sampler->getId()
 * (MinimalOptiX.cpp:444-479): RT_WRAP_REPEAT, normalized coordinates, RT_FILTER_LINEAR.  rgba holds
 * 4*w*h floats, row 0 = texture coordinate v 0 (the caller has already flipped the image as
 * MinimalOptiX.cpp:464 does).  *outTexId >= 1 goes into DisneyParams.albedoID; add textures before the
 * materials that name them. */
int moptix_add_texture(moptix_context ctx, const float* rgba, int32_t width, int32_t height, int32_t* outTexId);
int moptix_add_material(moptix_context ctx, const moptix_material* m, int32_t* outMatId);
/* createGeometry+sphereIntersect/sphereBBox+createGeometryInstance (MinimalOptiX.cpp:177-208,796-843) */
int moptix_add_spheres(moptix_context ctx, const moptix_sphere_params* s, const int32_t* matIds, int32_t n);
/* ...quadIntersect/quadBBox (MinimalOptiX.cpp:210-240, 505-510, 780-794) */
int moptix_add_quads(moptix_context ctx, const moptix_quad_params* q, const int32_t* matIds, int32_t n);
/* one tinyobj shape = one Geometry with six buffers (MinimalOptiX.cpp:392-441, Geometry.cu:114-119).
 * normals/texcoords may be NULL (count 0); nIdx/tIdx may be NULL or hold -1. */
int moptix_add_mesh(moptix_context ctx,
                    const float* positions, int32_t nVerts,
                    const float* normals, int32_t nNormals,
                    const float* texcoords, int32_t nTexcoords,
                    const int32_t* vIdx, const int32_t* nIdx, const int32_t* tIdx, int32_t nFaces,
                    int32_t matId);
/* context["lights"] buffer of LightParams (MinimalOptiX.cpp:523-531) */
int moptix_set_lights(moptix_context ctx, const moptix_light_params* lights, int32_t n);
/* rewrite sphere i..i+n (updateVideo, MinimalOptiX.cpp:763-764) */
int moptix_update_spheres(moptix_context ctx, int32_t first, const moptix_sphere_params* s, int32_t n);

/* setAcceleration("NoAccel" | "Trbvh") (MinimalOptiX.cpp:248,378,494,534,748).
 * "Trbvh" -> built on the device over all triangles: Morton order, then (option "builder" = 1, the default) a binned
 * surface-area-heuristic topology over that order, or (= 0) the Karras radix tree; four-wide 128-byte nodes either way.
 * Analytic primitives always stay in brute-force lists. "NoAccel" with triangles present
 * is rejected (MOPTIX_ERR_INVALID). */
int moptix_build_accel(moptix_context ctx, const char* kind);
int moptix_get_accel_info(moptix_context ctx, moptix_accel_info* out);
/* context->validate() (MinimalOptiX.cpp:542) */
int moptix_validate(moptix_context ctx);

/* ---- launch --------------------------------------------------------------- */
/* context["randSeed"]->setInt(seed); context->launch(0,W,H)  (MinimalOptiX.cpp:545-546,774-775):
 * one sample per pixel, accuBuffer += clamp(color,0,1); blocking. */
int moptix_launch(moptix_context ctx, int32_t randSeed);
/* the same nSeeds launches fused into ONE kernel (per pixel the samples are still
 * added in seed order, so the result is bit-identical to nSeeds moptix_launch calls). */
int moptix_render(moptix_context ctx, const int32_t* seeds, int32_t nSeeds);
/* non-blocking variant for stream overlap; moptix_sync() waits. */
int moptix_render_async(moptix_context ctx, const int32_t* seeds, int32_t nSeeds);
int moptix_sync(moptix_context ctx);
/* same work with the in-kernel counters enabled (slower; not for timing) */
int moptix_render_counted(moptix_context ctx, const int32_t* seeds, int32_t nSeeds, moptix_stats* out);

/* Multi-GPU tile split (new): this context renders one 8x8-pixel tile of every
 * group of nRanks tiles (raster order): tile g * nRanks + (rank + g) % nRanks of group g (the deal
 * rotates from group to group so that no rank owns whole columns).  Default (0,1) = whole frame. */
int moptix_set_partition(moptix_context ctx, int32_t rank, int32_t nRanks);

/* Multi-GPU collectives (new; SURVEY 8e, north_star "RCCL gather over xGMI"): one process per GPU, the context owns an
 * RCCL communicator.  One rank calls moptix_comm_unique_id (ncclGetUniqueId) and hands the 128 bytes to the others by
 * whatever the host has (a file, MPI, torch.distributed, a socket); every rank then calls moptix_comm_init
 * (collective: returns when all nRanks have called it).  Where the library offers it the communicator is NON-BLOCKING
 * (ncclCommInitRankConfig with config.blocking = 0; option "comm_blocking" = 1 asks for plain ncclCommInitRank): every RCCL call
 * then returns at once -- ncclInProgress while the library is still at work on the host, e.g. bringing a peer's connections up --
 * and this layer polls the communicator's state against "comm_timeout_ms".  With a blocking communicator a peer that is alive but
 * never makes its call holds the caller INSIDE ncclSend / ncclGroupEnd, where no deadline can reach.
 *   moptix_gather_tiles : tile split (moptix_set_partition(rank, nRanks) as the communicator's) -- every other rank packs its
 *                         tiles and ncclSend()s them to dstRank, which receives them in one group and writes them into its
 *                         accuBuffer on the device: dstRank then holds the whole frame, bit-identical to a one-GPU render.
 *   moptix_reduce_frame : sample split -- ncclReduce(sum) of the accuBuffers into dstRank's.
 * Both block until the data has landed -- at most "comm_timeout_ms" (option; default 120 s), host side (non-blocking communicator:
 * the call has not settled) and device side (its kernels have not finished) alike: a collective that has not completed by then (a peer
 * died or never called), or whose communicator reports an asynchronous error, is ABORTED (ncclCommAbort) and the call returns
 * MOPTIX_ERR_COMM; the host should exit.  The context stays usable as a one-rank context -- unless the dead collective's kernels
 * never leave its stream (a library without ncclCommAbort: the communicator is abandoned, not destroyed, and if the stream is still
 * busy after 10 s every later call on the context returns MOPTIX_ERR_COMM).  With a communicator of one rank they are no-ops.
 * moptix_pack_tiles / moptix_unpack_tiles are the device-side halves of the gather (rank r's tiles of the accuBuffer <->
 * a dense buffer of moptix_packed_tile_floats(nRanks) floats in work-item order), exposed so that the partition can be
 * tested on one GPU. */
#define MOPTIX_COMM_ID_BYTES 128
int moptix_comm_unique_id(uint8_t* id128);
int moptix_comm_init(moptix_context ctx, const uint8_t* id128, int32_t rank, int32_t nRanks);
int moptix_comm_destroy(moptix_context ctx);
int moptix_gather_tiles(moptix_context ctx, int32_t dstRank);
int moptix_reduce_frame(moptix_context ctx, int32_t dstRank);
int moptix_packed_tile_floats(moptix_context ctx, int32_t nRanks, uint64_t* outFloats);
int moptix_pack_tiles(moptix_context ctx, int32_t rank, int32_t nRanks, float* dstDevice);
int moptix_unpack_tiles(moptix_context ctx, int32_t rank, int32_t nRanks, const float* srcDevice);

/* The one option that is NOT a tuning knob:
 *   "shadow_rule"      1 (default): a shadow ray is decided by its NEAREST any-hit surface -- an opaque Disney surface gives (0,0,0), a
 *                      Disney GLASS surface gives its colour and nothing behind it is looked at.  This is DEVIATION D5' from SURVEY A2
 *                      ("an opaque surface anywhere on the segment blocks, every glass surface crossed multiplies"): it models what
 *                      OptiX does with disneyAnyHit (Material.cu:225-232 accepts the glass hit, which ends the ray's interval) under a
 *                      front-to-back traversal, and it is FITTED, not pinned: the evidence is the floor round the machine in
 *                      demo/coffee.png with a stand-in for the missing pot; real Trbvh traversal is not strictly front
 *                      to back.  0: SURVEY A2's order-independent rule (the oracle's switch shadow_any_opaque_blocks).  The two differ
 *                      only in scenes with a Disney GLASS material (the benchmark scene has none); takes effect at the next render.
 * tuning knobs.  The scheduler knobs (kernel_variant, slots_in_use, aux_depth, analytic_queue, tile_major, blocks_per_cu, swap_lanes,
 * starve_lanes, exit_threshold, leaf_threshold, sample_buffer_mb) never change a bit of the image.  The tree-shaping knobs (builder,
 * leaf_size, node_format) are bit-stable with ONE documented exception: the reference's float triangle test (Geometry.cu:121-160) can
 * accept a grazing hit on a needle triangle at a point outside that triangle's own bounding box, and whether any traversal ever tests
 * that triangle then depends on the boxes around it -- 1 pixel-sample in 3,600 fuzz cases (profiles/r04_fuzz.txt).
 * BOUND of that exception, as observed and as tests/test_gpu_parity.py::test_the_known_grazing_hit_is_tree_dependent_and_nothing_else replays it:
 * ONE pixel-sample of a frame takes another path (one closest hit more or less), every other pixel-sample keeps its bits; the frame's RMSE
 * against the oracle stays below north_star's 1e-3 (8e-4 on a 200x112 frame at 2 spp, i.e. below 1e-5 at any benchmark size).  It needs a
 * needle triangle and a ray within ~2e-4 of its plane; the benchmark scenes have shown none in 7,200 + 2,400 fuzz cases.
 *   "kernel_variant"   0 per-lane kernel, 3 path slots and queues shared by the workgroup (variants 1 and 2 of rounds 1-2 are gone),
 *                      4 = 3 with one shading visit per bounce (pt_packet.h; scenes with <= 3 lights, else 3 runs),
 *                      -1 (default) = the library's choice per launch: 4 for launches of >= 1e6 samples and >= 16 seeds
 *                      ("auto_packet" = 0 turns that off), else 3; scenes without triangles: see "analytic_queue" (they run a lean
 *                      instantiation of 3, four workgroups per CU).  get_option returns -1 while the choice is the library's
 *   "builder"          1 binned-SAH topology over the Morton order (default), 0 Morton radix tree
 *   "node_format"      variant 4: the node record the trace kernel fetches -- 128 = four child boxes in binary32 (one L2 line), 64 =
 *                      the same boxes on a 256-step grid over the node's box, rounded outwards (half a line: 4 L1 look-ups per
 *                      node step instead of 7, boxes up to a grid step larger), 0 (default) = whichever is cheaper for this scene
 *                      seen from this camera: decided at the first render after a build by walking one path per pixel of a
 *                      128-pixel-wide grid under both (get_option "node_format_used" tells the verdict)
 *   "slots_in_use"     path slots of a workgroup's pool (get_option "path_slots": 576 for variant 4, 512 for variant 3) that carry a
 *                      path (-1 = chosen per launch: 7/8 of them for variant 4 launches under 1e8 samples, else all); the others
 *                      are what deep paths borrow, see "aux_depth"
 *   "aux_depth"        variant 4: a path this deep (default 16; 0 = never) traces the shadow rays of each hit in slots
 *                      borrowed from finished paths, at the same time as the continuation ray (DESIGN.md "Borrowed slots").
 *                      A launch of 1e8 samples or more with "slots_in_use" left at -1 keeps no slot free to borrow and runs as
 *                      under 0, whatever the value
 *   "analytic_queue"   scenes without triangles: 1 = through the queue kernel, 0 = per-lane kernel, -1 (default) = queue
 *                      kernel from 64 primitives on
 *   "leaf_size"        1..8 triangles per BVH leaf (default 4; takes effect at the next build_accel)
 *   "tile_major"       hand-out order of the (pixel, sample) work items: 0 = sample-major, 1 = all samples of an
 *                      8x8 tile back to back, tiles with the deepest paths of earlier launches first,
 *                      2 = as 1 with one pixel's samples per wave, 3 = all samples of a pixel back to back, pixels with
 *                      the deepest paths of earlier launches first (default)
 *   "blocks_per_cu"    resident workgroups per CU (default 3)
 *   "swap_lanes", "starve_lanes"   node-loop swap / starvation thresholds of variants 3 and 4
 *   "exit_threshold", "leaf_threshold" (variant 0)
 *   "sample_buffer_mb" budget of the per-sample buffer (default 16384); larger batches run in passes
 *   "fast_shading"     0 (default): disneyPdf / disneyEval in correctly rounded binary32, bit-parity with the oracle;
 *                      1: hardware reciprocal / square-root approximations there (the reference itself is built with
 *                      -use_fast_math, utils_host.cpp:30-32): same rays, BRDF weights within ~1e-6, default kernel only
 *   "watchdog_ms"      wall-clock bound of one render kernel (default 600000); a pass cut short is not accumulated
 *   "comm_timeout_ms"  deadline of moptix_comm_init / moptix_gather_tiles / moptix_reduce_frame (default 120000): when the call has not
 *                      settled on the host or its kernels have not completed by then, or the communicator reports an asynchronous
 *                      error, the communicator is aborted and the call returns MOPTIX_ERR_COMM instead of blocking the rank for good
 *   "forget_history"   (write-only, any value) drop the per-pixel depth history that orders the work items ("tile_major"): the next launch
 *                      is ordered like the first one of a context -- what a single-frame render sees
 *   "comm_blocking"    1 = moptix_comm_init makes a blocking communicator even where a non-blocking one is available (default 0)
 *   "query_blocks_per_cu"  ray queries: the grid's cap in workgroups of 256 rays per CU (default 32, 1..64); a longer batch is walked by
 *                      that grid in a loop, and the stack overflow area is sized by it.  Time and memory only: same results for any value.
 *                      The radiance queries' grid has the same cap
 *   "radiance_buffer_mb"  radiance queries: the per-sample scratch a launch may use, in MB of 16-byte records (default 256, 1..16384); a
 *                      call with more samples runs in passes.  Time and memory only: same results for any value
 *   "drain_below"      variant 4: a workgroup of the trace kernel that is down to this many paths (default 64, 0 = never) hands them
 *                      to the drain kernel (csrc/drainkernel.hip: a wave per up to 16 paths, all lanes on one frontier) at their next
 *                      packet boundary and leaves; same image bits, ray and hit counts either way -- the node / triangle-test counts
 *                      of a counted launch then vary a little from run to run (the frontier's visiting order follows its atomics).  The one
 *                      documented exception to order independence -- a grazing hit outside its triangle's own box, below -- can in principle
 *                      make a drained path's result depend on that order; no such case in 3,300 fuzz cases with the drain kernel on
 *   "specialize"       variant 4: 1 (default) = a scene whose tables hold no textured material, no sphere light, no Lambertian / metal /
 *                      glass material and no analytic sphere is traced by a build of the trace kernel without those programs; 0 = always
 *                      the general build.  Decided at every launch from the tables as they are then; same image bits either way
 * read-only (get_option): "kernel_variant_used", "kernel_features_used" (the programs compiled into the last launch's trace kernel:
 *   1 textures | 2 sphere lights | 4 Lambertian / metal / glass | 8 analytic spheres; 15 = the general build, 0 = the lean one), "kernel_slim_used" (1: the last launch ran the lean
 *   build without borrowed slots and, unless shadow rays keep their nearest candidate, without Disney GLASS; else 0), "node_format_used", "path_slots", "num_cus", "comm_ranks" (size of the context's
 *   communicator, 0 without one), "comm_nonblocking_used" (1: that communicator is non-blocking), and after moptix_render_counted
 *   "counted_span_us" (first wave in -> last wave out of the trace kernel) / "counted_tail_us" (the part of it after the last
 *   work item was handed out: the launch's drain; -1 for the per-lane kernel)
 * Unknown names -> MOPTIX_ERR_INVALID. */
int moptix_set_option(moptix_context ctx, const char* name, int32_t value);
int moptix_get_option(moptix_context ctx, const char* name, int32_t* value);

/* ---- output buffer: createBuffer(RT_BUFFER_INPUT_OUTPUT, FLOAT3, W, H) + map()/unmap()
 *      (MinimalOptiX.cpp:144-147, 44-60).  float3 row-major, row 0 = bottom row. -- */
int moptix_accum_read(moptix_context ctx, float* dstHost);          /* W*H*3 floats */
int moptix_accum_clear(moptix_context ctx);
int moptix_accum_device_ptr(moptix_context ctx, void** devPtr);     /* for device-side gather/reduce */
/* render into caller-owned device memory (e.g. a torch tensor) instead; NULL restores the own buffer */
int moptix_accum_bind(moptix_context ctx, void* devPtr);
/* updateContent (MinimalOptiX.cpp:43-66) on the device: out[(H-1-y)*W+x] = u8(clamp(accu/n,0,1)*255),
 * optionally clearing the accumulator. dstHost: W*H*3 bytes, row 0 = top. */
int moptix_resolve_rgb8(moptix_context ctx, float nAccumulation, int clearBuffer, uint8_t* dstHost);

/* ---- first-hit AOVs (new): guide layers for a denoiser, depth and ids for compositing / picking / masks ----------------
 * For every pixel of the WHOLE frame (whatever moptix_set_partition says) and each seed s of the call, the primary ray the beauty
 * pass traces for (pixel, s) -- the same origin on the lens, the same jitter -- is traced to its closest hit (rule D5: nearest t,
 * then the lower primitive id), and per-pixel float32 sums are added to, in seed order:
 *   buffer         per sample                                                                        on a miss
 *   albedo (3)     colour of the hit's program: Lambertian / metal / glass -> albedo; Disney         bgColor
 *                  non-glass -> Cdlin (srgb2lin of the texel when textured); Disney glass -> the
 *                  tint of its refraction (colour or raw texel); light -> clamp(emission, 0, 1)
 *   normal (3)     faceforward(shading normal, -d, geometric normal): world space, facing the camera (0,0,0)
 *   depth (1)      t of the hit (distance along the normalised direction from the lens point)       nothing
 *   hits (1)       1                                                                                 nothing
 *   primId, matId  (int32) primitive id (spheres, quads, triangles in upload order, as               -1
 *                  moptix_debug_trace reports it) and material of the hit -- from the first sample
 *                  after a clear only
 * Layout as the accumulation buffer: row 0 = bottom row, RGB triples interleaved.  Calls accumulate until moptix_aov_clear: seed
 * lists A then B give the bits of one call with A + B; moptix_aov_samples counts the seeds added since the clear (divide by it;
 * depth by hits).  A change of frame size in moptix_set_params clears them.  The buffers are allocated at the first AOV call.
 * An AOV call changes nothing else: not the accumulation buffer, the depth history that orders work items ("tile_major"), the
 * node-format verdict, moptix_kernel_time / moptix_reduce_time or the counters of a counted render.  The 64-byte nodes are walked
 * where the tree has them, the 128-byte ones where it has not or where option "node_format" is 128 (same hits: rule D5; the one
 * documented tree-dependent grazing hit applies, see the options below).
 *   moptix_render_aovs  blocking; adds nSeeds samples (MOPTIX_ERR_STATE before params + build_accel)
 *   moptix_aov_read     copies the buffers to host memory: W*H*3 floats (albedo, normal), W*H floats (depth, hits), W*H int32
 *                       (primId, matId); NULL members are skipped
 *   moptix_aov_bind     caller-owned device memory (e.g. torch tensors) of the same sizes instead of the own buffers; a NULL member
 *                       keeps the own buffer of that AOV, a NULL argument restores all of them.  The sample count restarts at 0 and
 *                       the bound memory is taken as it is: call moptix_aov_clear before the first render into it. */
typedef struct moptix_aov_buffers { float *albedo, *normal, *depth, *hits; int32_t *primId, *matId; } moptix_aov_buffers;
int moptix_render_aovs(moptix_context ctx, const int32_t* seeds, int32_t nSeeds);
int moptix_aov_clear(moptix_context ctx);
int moptix_aov_samples(moptix_context ctx, uint64_t* out);
int moptix_aov_read(moptix_context ctx, const moptix_aov_buffers* dstHost);
int moptix_aov_bind(moptix_context ctx, const moptix_aov_buffers* dstDevice);

/* ---- denoiser (new): edge-aware a-trous filter guided by the first-hit AOVs -------------------------------------------------
 * The edge-avoiding a-trous wavelet transform (Dammertz et al. 2010) with SVGF's luminance-variance edge stop (Schied et al. 2017),
 * spatial part (the temporal part is moptix_denoise_temporal below).  Inputs per pixel p (row 0 = bottom, the accumulation buffer's layout), S = moptix_aov_samples:
 *   C_p = accum_p / nAccumulation      the beauty mean (nAccumulation as in moptix_resolve_rgb8)
 *   A_p = albedo_p / S,  N_p = normalize(normal_p / S) (0 where that is 0),  Z_p = depth_p / hits_p
 * p is a geometry pixel iff hits_p > 0.  A background pixel (hits 0) outputs C_p bit for bit and is never a tap.
 * Demodulation (demodulate = 1): the filter works on I_p = C_p / max(A_p, 1e-3) per channel and outputs I'_p * max(A_p, 1e-3);
 * demodulate = 0 (the default): I = C.  The albedo AOV is the first hit's program colour, which on coffee's metal, glass and
 * near-zero albedo channels is far from what the beauty reflects: demodulated, 4 spp there come out 3.7x worse than undenoised
 * (DESIGN.md "Denoiser").
 * Prepass: luminance l(I) = 0.2126 r + 0.7152 g + 0.0722 b.  Variance v_p = E[l^2] - E[l]^2 (biased) of l over the geometry pixels
 * of the 3x3 window, clamped at 0.  Depth gradient g_p = max over the two axes of |Z+ - Z-| / 2 (both neighbours geometry),
 * |Z_n - Z_p| (one of them), 0 (none).
 * Iteration i = 0 .. L-1, step = 2^i, taps q = p + step (dx, dy), dx, dy in -2..2; taps outside the frame or on background skipped:
 *   w   = h(dx) h(dy) w_n w_z w_l,  h = (1/16, 1/4, 3/8, 1/4, 1/16)
 *   w_n = max(0, N_p . N_q)^normalPower  (integer power by binary exponentiation, least significant bit first:
 *         r = 1, b = x; loop { if (n & 1) r = r * b; n >>= 1; if (n == 0) stop; b = b * b; } -- no powf)
 *   w_z = exp(-|Z_p - Z_q| / (sigmaDepth * step (|dx| + |dy|) * g_p + 1e-4))
 *   w_l = exp(-|l_p - l_q| / (sigmaLuminance * sqrt(G3(v)_p) + 1e-4)),  G3 = the 3x3 (1/4, 1/2, 1/4) blur of v over geometry pixels
 *   I'_p = sum w I_q / sum w,  v'_p = sum w^2 v_q / (sum w)^2
 *   the centre tap has w = h(0)^2 = 9/64 (its w_n, w_z, w_l are 1), so sum w > 0 even where N_p cancelled to 0; taps are summed in
 *   row-major order (dy outer, dx inner) with plain adds.
 * iterations = 0 returns C bit for bit (no demodulation).  Arithmetic: the contract of csrc/pt_math.h (AC1-AC5, no contraction);
 * exp is exp_ac (csrc/pt_denoise.h: Cody-Waite reduction by ln 2 with fma, a fixed polynomial, 2^k from its bits; 0 below x = -87,
 * exactly 1 at 0); no libm transcendental, so that host and device give the same bits.
 * Ranges: iterations 0..8 (default 5), normalPower 1..256 (128), demodulate 0 / 1 (0), sigmaLuminance >= 0 (4), sigmaDepth >= 0 (1),
 * finite; nAccumulation > 0.  Bad values -> MOPTIX_ERR_INVALID.
 *   moptix_denoise_defaults  the defaults above; pure host (works without a device)
 *   moptix_denoise           blocking, on the context's stream (moptix_set_stream).  MOPTIX_ERR_STATE before moptix_set_params or
 *                            while moptix_aov_samples is 0 (e.g. after a frame-size change, until AOVs are rendered again).  Reads
 *                            the accumulation buffer and the AOVs wherever they are bound and changes nothing else: not those
 *                            buffers or the AOV sample count, the depth history, the node-format verdict, moptix_kernel_time /
 *                            moptix_reduce_time.  Scratch and output are allocated at the first call, freed by a frame-size change
 *                            and by moptix_destroy.
 *   moptix_denoise_read      copies the output to host memory: W*H*3 floats in the accumulation buffer's layout (MOPTIX_ERR_STATE
 *                            when nothing was denoised since the last frame-size change)
 *   moptix_denoise_bind      caller-owned device memory of W*H*3 floats that later calls write instead of the own buffer; NULL
 *                            restores the own buffer.  The binding survives a frame-size change: the caller sizes the memory.
 * Tile split (moptix_set_partition): the accumulation buffer holds this rank's tiles only -- call the denoiser on the destination rank
 * of moptix_gather_tiles, after the gather. */
typedef struct moptix_denoise_params {
  int32_t iterations, normalPower, demodulate;
  float sigmaLuminance, sigmaDepth;
} moptix_denoise_params;
int moptix_denoise_defaults(moptix_denoise_params* out);
int moptix_denoise(moptix_context ctx, const moptix_denoise_params* p, float nAccumulation);
int moptix_denoise_read(moptix_context ctx, float* dstHost);
int moptix_denoise_bind(moptix_context ctx, float* dstDevice);

/* ---- denoiser: temporal accumulation with reprojection (new) ------------------------------------------------------------------
 * moptix_denoise_temporal does what moptix_denoise does with SVGF's temporal stage in front of the a-trous iterations and a history
 * kept in the context between calls.  Per call (frame k), with C, A, N, Z, hits decoded as above (demodulation as there; iterations =
 * 0 runs without demodulation, as moptix_denoise) and primId, matId from the AOV buffers; W, H the frame size:
 * 1 World point.  Geometry pixel p = (x, y): u = (x + 0.5) / W, v = (y + 0.5) / H,
 *     t = ((scrLowerLeftCorner + u * horizontal) + v * vertical) - origin per component, d = normalize(t), P = fma(Z_p, d, origin):
 *     the pinhole ray through the pixel centre (with lensRadius > 0 an approximation that the validity tests below absorb).
 * 2 Object motion.  primId_p < nSpheres (ids are spheres, quads, triangles in upload order): P' = P - (center_now - center_prev) of
 *     that sphere per component, else P' = P.  "prev" centres and camera are those the context held (its host copy of the spheres, the
 *     camera of moptix_set_params) at the end of the previous moptix_denoise_temporal call; moptix_update_spheres is not hooked.
 *     Triangles, with the option "temporal_face_motion" = 1 (moptix_set_option; 0, the default, leaves a moved triangle to the validity
 *     tests of step 4 and gives the bits this entry gave before the option existed).  f = primId_p - nSpheres - nQuads is the pixel's
 *     face (moptix_update_faces' numbering); the case applies when 0 <= f < nTracked, the number of faces on the device for which a
 *     snapshot exists.  "now" positions p0 p1 p2 of the face: the device copy of the faces as it stands when the call runs, whether or
 *     not a refit has followed the last update -- so denoise a frame BEFORE updating the faces for the next one.  "prev": what the
 *     device copy held at the end of the previous moptix_denoise_temporal call made with the option on.  d_i = p_i(now) - p_i(prev)
 *     per component, one binary32 subtraction each.  All nine components zero: the face has not moved, its motion is (0, 0, 0) and the
 *     pixel takes the path of a static one (the exact shortcut of step 3 included), so a static mesh gives the same bits with the
 *     option on.  Otherwise, with e1 = p1 - p0, e2 = p2 - p0, n = cross(e1, e2), nn = dot(n, n), w = P - p0:
 *       nn > 0:  bu = dot(cross(w, e2), n) / nn,  bv = dot(cross(e1, w), n) / nn, each clamped to [-1, 2] (max, then min);  else bu = bv = 0
 *       mo = (d0 + bu * (d1 - d0)) + bv * (d2 - d0) per component, in this order;  P' = P - mo
 *     -- the triangle's own affine motion at the projection of P onto its plane; the clamp bounds the extrapolation at silhouettes,
 *     where the mean depth and the first sample's primId disagree.  Quads are not reprojected.
 *     Snapshot life: taken by every call with the option on; dropped by moptix_clear_scene, by a different number of faces on the
 *     device (faces added, then a rebuild), by setting the option to 0 and by everything that drops the history (step 8).  A call
 *     without a usable snapshot treats every face as unmoved and takes the snapshot; a changed face count does not drop the history.
 *     moptix_build_accel over the same number of faces keeps the snapshot: the faces keep their upload order.  The per-face pass runs
 *     only in a call before which moptix_update_faces*, moptix_build_accel or moptix_clear_scene ran: a static scene pays nothing.
 * 3 Projection into the previous camera (o', LL', H', V').  a = LL' - o', b = H', c = V', r = P' - o'; Cramer's rule on
 *     r = s a + (s u') b + (s v') c with the triple products written as dots with cross(b, c), cross(c, a), cross(a, b) (AC1, AC2):
 *     det = dot(a, cross(b, c)), sn = dot(r, cross(b, c)), s = sn / det; det == 0 or not s > 0 -> no history;
 *     u' = dot(r, cross(c, a)) / sn, v' = dot(r, cross(a, b)) / sn; previous continuous pixel (fx, fy) = (u' W - 0.5, v' H - 0.5),
 *     expected previous depth Z' = length(r).  Where the previous camera is this one bit for bit (origin, horizontal, vertical,
 *     scrLowerLeftCorner) and the pixel's object motion is (0, 0, 0), (fx, fy) = (x, y) and Z' = Z_p exactly: a static pixel maps onto
 *     itself.  No history unless -1 < fx < W and -1 < fy < H.  Motion vector of the pixel: (x - fx, y - fy); (0, 0) without history.
 * 4 Taps and validity.  x0 = floor(fx), tx = fx - x0 (y alike); taps (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), in this
 *     order, with weights (1 - tx)(1 - ty), tx (1 - ty), (1 - tx) ty, tx ty.  A tap q counts iff its weight is > 0, it is inside the
 *     frame, was a geometry pixel in the previous frame, matId_prev(q) == matId_p, N_p . N_prev(q) >= normalThreshold and
 *     |Z_prev(q) - Z'| <= depthTolerance * Z'.  Sums over the counted taps with plain adds: sw = sum w, sum w I_q per channel,
 *     sum w m1_q, sum w m2_q; each is divided by sw once (renormalisation).  No counted tap, or sw < 1e-2 -> disocclusion.
 * 5 Accumulate.  h = min(min over counted taps of h_q + 1, maxHistory); h = 1 on disocclusion and on a background pixel.
 *     alpha_h = max(1 / h, alpha) (1 / h one binary32 division); I_acc = I_prev + alpha_h * (I - I_prev) per channel; the luminance
 *     moments m1, m2 of l = l(I), l * l likewise with max(1 / h, alphaMoments).  Disocclusion: I_acc = I, m1 = l, m2 = l * l.  The history
 *     is this PRE-FILTER accumulation.
 * 6 Variance.  h >= varianceFrames: v = max(0, m2 - m1 * m1); otherwise the prepass's 3x3 spatial estimate, taken on I_acc.  The depth
 *     gradient g is the prepass's.
 * 7 Filter and output.  The L iterations and the final pass of moptix_denoise on {I_acc, v}, into the denoiser's output:
 *     moptix_denoise_read / moptix_denoise_bind serve both entries.  iterations = 0 outputs I_acc.  Background pixels output C bit for
 *     bit, keep h = 1 and never serve as taps.
 * 8 History life.  Stored after each call: {I_acc, h}, {m1, m2}, the frame's {N, Z} and matId, the camera, the sphere centres.  Dropped
 *     -- the next call behaves as a first frame, every pixel h = 1 -- by moptix_temporal_reset, a change of frame size, a different
 *     sphere count, moptix_clear_scene, and a change of the demodulation in effect (demodulate, or iterations going to or from 0 with
 *     demodulate = 1).  The first call after a drop gives, for varianceFrames > 1, the bits of moptix_denoise with the same parameters.
 * Arithmetic as the denoiser's (csrc/pt_temporal.h states every operation in order).  Ranges: alpha, alphaMoments in [0, 1] (0.2, 0.2),
 * depthTolerance >= 0 (0.2), normalThreshold in [-1, 1] (0.5), finite; maxHistory 1..65536 (32), varianceFrames 1..65536 (4).  Bad
 * values -> MOPTIX_ERR_INVALID; state errors and the other argument checks as moptix_denoise.
 *   moptix_temporal_defaults  the defaults above; pure host
 *   moptix_denoise_temporal   blocking, on the context's stream.  Like moptix_denoise it reads the accumulation buffer and the AOVs
 *                             (primId and matId too) wherever they are bound and changes nothing else in the context.  The history
 *                             (two sets of three float4 per pixel) is allocated at the first call, freed by a frame-size change and
 *                             by moptix_destroy.
 *   moptix_temporal_reset     drops the history
 *   moptix_temporal_info      frames = calls since the last drop; of the last call: geometry pixels, geometry pixels that found
 *                             history, geometry pixels that did not (disoccluded; all of them in a first frame), and the mean h over
 *                             the geometry pixels (integer sums reduced on the device)
 *   moptix_temporal_read      of the last call: motion vectors (W*H*2 floats, x then y) and history lengths h (W*H floats), in the
 *                             accumulation buffer's pixel order; NULL members are skipped (MOPTIX_ERR_STATE when there was no call
 *                             since the last frame-size change)
 *   moptix_temporal_face_info of the last call: trackedFaces = faces with a usable snapshot in that call (0 with the option off and in
 *                             a call that only took the snapshot), movedFaces = tracked faces with a non-zero displacement,
 *                             movedPixels = geometry pixels whose face was a moved one (integer sums reduced on the device); zeros
 *                             before the first call.  The snapshot, three float4 per face of displacement records and the counters
 *                             are allocated at the first call that needs them and freed with the snapshot and by moptix_destroy. */
typedef struct moptix_temporal_params {
  float alpha, alphaMoments, depthTolerance, normalThreshold;
  int32_t maxHistory, varianceFrames;
} moptix_temporal_params;
typedef struct moptix_temporal_stats {
  uint64_t frames, geometryPixels, historyPixels, disoccludedPixels;
  float meanHistory;
} moptix_temporal_stats;
typedef struct moptix_temporal_buffers { float *motion, *history; } moptix_temporal_buffers;
int moptix_temporal_defaults(moptix_temporal_params* out);
int moptix_denoise_temporal(moptix_context ctx, const moptix_denoise_params* p, const moptix_temporal_params* t, float nAccumulation);
int moptix_temporal_reset(moptix_context ctx);
int moptix_temporal_info(moptix_context ctx, moptix_temporal_stats* out);
int moptix_temporal_read(moptix_context ctx, const moptix_temporal_buffers* dstHost);
typedef struct { uint64_t trackedFaces, movedFaces, movedPixels; } moptix_temporal_face_stats;
int moptix_temporal_face_info(moptix_context ctx, moptix_temporal_face_stats* out);

/* ---- adaptive sampling (new): per-pixel sample counts and luminance moments, and a render that stops sampling converged pixels ----
 * moptix_render_adaptive renders a list of seeds like moptix_render, but after a first pass over the whole frame it keeps sampling
 * only the pixels whose estimated error is above a threshold.  Whole frame only: with a tile split (moptix_set_partition other than
 * (0, 1)) a pixel's 3x3 window crosses into other ranks' tiles and the call returns MOPTIX_ERR_STATE.
 * Per-pixel state, in the accumulation buffer's pixel order (row 0 = bottom), allocated at the first adaptive call:
 *   count      uint32      samples added to the pixel since the clear
 *   moments    2 float32   s1 = sum l, s2 = sum l * l over those samples, plain binary32 adds in seed order; l = 0.2126 r + 0.7152 g +
 *                          0.0722 b as the denoiser's l(I) (same operation order), of the clamped colour the trace kernel stored
 *   converged  uint8       sticky: set once, cleared by moptix_adaptive_clear only
 * Error of a pixel with n = count > 0: m = s1 / n, v = max(0, s2 / n - m * m) (biased), e = sqrt(v / n) / (m + 0.01) -- the relative
 * standard error of the mean luminance with a floor of about 2.5 / 255; e = 0 where n = 0.  Every operation is one correctly rounded
 * binary32 operation in the order written (n converted to float once; csrc/pt_adaptive.h).
 * After each pass, for every pixel that is not converged: needs = n < minSamples || max of e over the in-frame pixels of its 3x3
 * window > threshold; a pixel that does not need more becomes converged.  threshold == 0 means "no pixel converges".
 * Passes: pass 0 takes the first min(minSamples, nSeeds) seeds, every later pass up to `batch` seeds, until the seeds are used up or
 * no pixel is active.  A pixel active in a pass gets ALL seeds of that pass, so every pixel's samples are a prefix of the seed list:
 *   accum[p] has the bits that moptix_render(seeds[0 : count[p]]) on a cleared accumulator leaves in accum[p],
 * and with threshold = 0 the accumulation buffer has the bits of moptix_render(seeds), count == nSeeds everywhere.  The budget of the
 * per-sample buffer ("sample_buffer_mb") cuts a pass into sub-passes as it cuts moptix_render's; per pixel nothing changes.
 * A second call without a clear continues: the new seeds go to the pixels still active, counts and moments keep adding, and it has no
 * minSamples pass of its own when the state already holds a pass (every pass is then up to `batch` seeds).  Seed lists A then B with
 * the same parameters give the bits of one call with A + B WHEN A's length is a pass boundary of the joint call (minSamples + j *
 * batch), not otherwise.
 * The passes run through a trace kernel that keeps its paths in slots, handing the work out by pixel ("tile_major" 3), whatever the
 * options "tile_major", "kernel_variant" and "analytic_queue" say: where moptix_render would take the per-lane kernel the queue kernel
 * runs (get_option "kernel_variant_used" tells).  The kernels give the same bits (see the options), so this changes time only; the
 * options read back as the caller set them.  The depth history that orders work items keeps being updated and is restarted per pixel
 * when it was kept per tile.
 * The counts describe what is in the accumulation buffer, so the two cannot be mixed silently:
 *   - moptix_accum_clear, moptix_accum_bind, a clearing moptix_resolve_rgb8 and a change of frame size drop the adaptive state (it is
 *     zeroed at the next adaptive call; bound memory is taken as it is: moptix_adaptive_clear before the first adaptive render into it);
 *   - moptix_launch / moptix_render / moptix_render_async / moptix_render_counted after an adaptive call without a clear in between
 *     return MOPTIX_ERR_STATE, and so does moptix_render_adaptive on an accumulator that those, moptix_unpack_tiles, moptix_gather_tiles
 *     (on the destination rank) or moptix_reduce_frame have written to since its last clear.
 * Ranges: threshold >= 0 and finite (default 0.03), minSamples >= 1 (16), batch >= 1 (64: every pass ends in the
 * tail of its deepest paths, and sixteen passes of 16 seeds cost a 1920x1080 frame 45 % more than one of 256); bad values -> MOPTIX_ERR_INVALID.
 *   moptix_adaptive_defaults      the defaults above; pure host (works without a device)
 *   moptix_render_adaptive        blocking, on the context's stream; `out` may be NULL.  Stats: passes and samplesTraced of this call,
 *                                 samplesUniform = in-frame pixels x nSeeds, and after the last pass the pixels still active, the
 *                                 converged pixels, the smallest and largest count
 *   moptix_adaptive_clear         zeroes count, moments, converged AND the accumulation buffer
 *   moptix_adaptive_read          copies count (W*H uint32), moments (W*H*2 floats), error (W*H floats: e as defined, as of the last
 *                                 pass) and converged (W*H bytes) to host memory; NULL members are skipped.  MOPTIX_ERR_STATE when
 *                                 there is no adaptive state at this frame size (the reading entry points below alike)
 *   moptix_adaptive_mean          W*H*3 floats: accum / count per pixel and channel (one division each), 0 where count is 0
 *   moptix_adaptive_mean_device   the same into caller-owned device memory (e.g. the accumulator of a denoise call with nAccumulation 1)
 *   moptix_adaptive_resolve_rgb8  moptix_resolve_rgb8's clamp, rounding and row flip on that mean; W*H*3 bytes, row 0 = top
 * An adaptive call changes nothing else: not the AOVs, the denoiser's output, the temporal history or the node-format verdict. */
typedef struct moptix_adaptive_params { float threshold; int32_t minSamples, batch; } moptix_adaptive_params;
typedef struct moptix_adaptive_stats {
  uint64_t passes, samplesTraced, samplesUniform;
  uint64_t activePixelsLast, convergedPixels;
  uint32_t minCount, maxCount;
} moptix_adaptive_stats;
typedef struct moptix_adaptive_buffers { uint32_t* count; float *moments, *error; uint8_t* converged; } moptix_adaptive_buffers;
int moptix_adaptive_defaults(moptix_adaptive_params* out);
int moptix_render_adaptive(moptix_context ctx, const int32_t* seeds, int32_t nSeeds, const moptix_adaptive_params* p, moptix_adaptive_stats* out);
int moptix_adaptive_clear(moptix_context ctx);
int moptix_adaptive_read(moptix_context ctx, const moptix_adaptive_buffers* dstHost);
int moptix_adaptive_mean(moptix_context ctx, float* dstHost);
int moptix_adaptive_mean_device(moptix_context ctx, float* dstDevice);
int moptix_adaptive_resolve_rgb8(moptix_context ctx, uint8_t* dstHost);

/* ---- ray queries (new): closest hit and occlusion for the caller's own rays ---------------------------------------------------
 * A ray is eight floats  ox oy oz dx dy dz tmin tmax  (moptix_debug_trace's layout).  The direction is used as given, not normalised;
 * t is in units of |d| (the sphere intersector solves the unit-direction quadratic, as for every ray of the renderer: give spheres
 * unit directions).  Needs moptix_set_params and moptix_build_accel like a render; the camera and the frame size play no part.
 * MOPTIX_QUERY_CLOSEST -> one moptix_hit (32 bytes) per ray:
 *   t     distance along the ray of the nearest primitive: nearest by (t, prim) among the primitives the ray meets with
 *         tmin < t < tmax; at exactly equal t the lower prim wins (rule D5), so the answer depends neither on the tree nor on the
 *         node format nor on scheduling.  Every primitive counts, whatever its material (lights and glass included).
 *   prim  primitive id: spheres, then quads, then triangles by original face id (what moptix_debug_trace reports); -1 = miss
 *   mat   material id of the primitive; -1 on a miss
 *   u, v  triangles: the barycentric weights of the face's second and third vertex (the hit point is p0 + u (p1 - p0) + v (p2 - p0));
 *         0 for spheres and quads
 *   ng    geometric normal as the closest-hit programs receive it, before any face-forward flip: triangles normalize(cross(p0 - p2,
 *         p1 - p0)), spheres normalize(hit point - centre), quads the plane's normal
 *   miss  t = tmax, prim = mat = -1, every other field 0
 * MOPTIX_QUERY_ANY -> one int32 per ray: 1 if and only if the closest query on the same ray reports prim >= 0, else 0.  Purely
 * geometric (the shadow rays' material classes, "shadow_rule" and Disney glass play no part); the traversal stops at the first
 * primitive it accepts.
 * Invalid rays are misses, decided before traversal: a non-finite component, tmax <= tmin, or a zero direction.  A negative tmin is
 * walked as tmin = 0 (the traversal works on t >= 0, which is why moptix_set_params refuses a negative rayEpsilonT): nothing behind the
 * origin is reported.
 * Nodes: the 64-byte form where the tree has one, else the 128-byte one; option "node_format" 64 / 128 forces either (same bits).
 *   moptix_query_rays_device  dRays, dOut: device memory, 16-byte aligned (dOut of MOPTIX_QUERY_ANY: 4).  Asynchronous on the
 *                             context's stream (moptix_set_stream): moptix_sync, or the stream's own synchronisation, waits for
 *                             it.  Allocates nothing after the first query on a tree: the stack overflow area
 *                             lives in the context until moptix_clear_scene, moptix_build_accel or moptix_destroy.  The scene tables
 *                             are read as they are when the kernel runs: a query after moptix_update_spheres sees the moved spheres.
 *   moptix_query_rays         host pointers, blocking: upload, query, read back (staging kept in the context)
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 rays); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_render.  A query changes nothing else in the context. */
typedef struct { float t; int32_t prim; int32_t mat; float u, v; float ng[3]; } moptix_hit;
enum { MOPTIX_QUERY_CLOSEST = 0, MOPTIX_QUERY_ANY = 1 };
int moptix_query_rays_device(moptix_context ctx, const float* dRays, int64_t n, int32_t mode, void* dOut);
int moptix_query_rays(moptix_context ctx, const float* rays, int64_t n, int32_t mode, void* out);

/* ---- multi-hit ray queries: the first maxHits hits along each ray, in order ---------------------------------------------------------
 * Everything a ray passes through: the thickness of a wall, the entry / exit intervals of a solid, the layers behind a surface, a crossing
 * count as an inside test for meshes that are not closed -- in one walk, and right at exactly equal t, where re-launching closest
 * queries with an advanced tmin skips the second of two coincident surfaces.
 * A ray is the ray queries' eight floats, valid or invalid by their rule; a negative tmin is walked as 0.
 * The hit set H of a valid ray is the set of pairs (t, prim) over every primitive record whose own test accepts it with tmin < t < tmax:
 * a triangle or a quad gives at most one pair; a sphere one per root inside the interval, so a sphere entered and left gives two pairs
 * with the same prim and a tangent ray (both roots equal) one.  Every primitive counts, whatever its material.  An invalid ray has
 * H = {}.  H is a function of the ray and the device records alone.
 *   hits    n x maxHits moptix_hit records, ray-major.  For ray i the first c = min(maxHits, |H|) records are the c least elements of H by
 *           (t, prim) ascending (rule D5's order), each filled exactly as MOPTIX_QUERY_CLOSEST fills a closest hit at that (t, prim):
 *           mat, u, v and ng before any face-forward flip -- a sphere's exit hit has the outward normal, which points along the ray.
 *           Records c .. maxHits - 1 are miss records (t = the given tmax, prim = mat = -1, the rest 0).  Every byte is defined.  Record
 *           0 has the bits of MOPTIX_QUERY_CLOSEST on the same ray.
 *   counts  n x int32: c.  With MOPTIX_MULTI_COUNT_ALL: |H|, the number of crossings -- the walk then cannot prune and visits every box
 *           the ray meets inside (tmin, tmax), which costs well above a closest query.  counts[i] > 0 if and only if MOPTIX_QUERY_ANY
 *           gives 1 on the same ray.
 *   maxHits 1..64.  With MOPTIX_MULTI_COUNT_ALL also 0, and hits may then be NULL: the pure crossing count.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part, with the one exception the closest query
 * has: a grazing hit that the triangle test accepts outside the triangle's own padded box is not seen by a walk that never enters that
 * box.  Here that holds for every triangle along the ray, not only for the nearest.
 *   moptix_query_rays_multi_device  dRays, dHits: device memory, 16-byte aligned; dCounts: device memory, 4-byte aligned.  Asynchronous on
 *                                   the context's stream.  While a ray is walked its slice of dHits holds the candidates; nothing else
 *                                   is allocated or written.  It uses the ray queries' stack overflow area (same grid cap, allocated at
 *                                   the first ray query of either kind on a tree): moptix_debug_buffer_addresses out[0] keeps its value
 *                                   across a multi-hit query.
 *   moptix_query_rays_multi         host pointers, blocking: upload, query, read back (the ray queries' staging)
 * n may be any int64 >= 0: longer batches are cut into launches of floor(2^30 / max(maxHits, 1)) rays, so that a launch writes at most
 * 2^30 records and a record's index within it fits an int as a ray's does; n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or misaligned
 * pointers, n < 0, maxHits out of range, unknown flag bits; state errors as moptix_query_rays ("faces dirty" before a refit included).
 * A multi-hit query changes nothing else in the context. */
enum { MOPTIX_MULTI_COUNT_ALL = 1 };
int moptix_query_rays_multi_device(moptix_context ctx, const float* dRays, int64_t n, int32_t maxHits, uint32_t flags,
                                   void* dHits, int32_t* dCounts);
int moptix_query_rays_multi(moptix_context ctx, const float* rays, int64_t n, int32_t maxHits, uint32_t flags,
                            moptix_hit* hits, int32_t* counts);

/* ---- radiance queries: path-traced radiance for the caller's own rays -------------------------------------------------------------
 * How much light arrives along a ray, from the materials, lights, next-event estimation and shadow rule the frame uses: a probe, a
 * lightmap texel, another sensor model.  The camera and the frame size play no part; "fast_shading" is not consulted.
 * A ray is the ray queries' eight floats  ox oy oz dx dy dz tmin tmax, valid or not by their rule (a non-finite component, tmax <= tmin
 * or a zero direction: invalid; a negative tmin is walked as 0).  THE DIRECTION MUST BE UNIT LENGTH: it is used as given, the shading
 * code assumes |d| = 1 and nothing renormalises it.  The ray's own tmin and tmax hold for its first segment only; every later segment
 * of the path is the renderer's (rayEpsilonT and so on).
 * Each ray gets nSamples samples, one path each.  The RNG state a path starts from:
 *   seeds    nSamples launch seeds (host memory, copied): sample s of ray i starts from tea16(uint32(indexBase + i), uint32(seeds[s])),
 *            the camera's rule with the ray's index in the pixel's place; indexBase wraps mod 2^32.  A query cut into calls on ranges
 *            of the rays, each with indexBase = its first ray's index, equals the one call.
 *   states   n x nSamples words, ray-major: sample s of ray i starts from states[i * nSamples + s], taken as it is.
 * Exactly one of the two is given.  The path then runs as a camera path does from depth 1, throughput (1,1,1): rayMaxDepth, bgColor,
 * the lights and "shadow_rule" act as in a render.  A sample's value is its radiance, unclamped; with MOPTIX_RADIANCE_CLAMP each channel
 * is clamped to [0, 1] as a frame's samples are (then a camera's rays and the states its lens and jitter draws leave behind reproduce
 * the accumulation buffer of moptix_render bit for bit).
 * Output: four floats  r g b t  per ray.
 *   r g b  the binary32 sum of the ray's sample values in sample order, from +0, by plain adds -- not divided by nSamples.  The bits
 *          depend neither on the scheduling nor on "query_blocks_per_cu", "radiance_buffer_mb" or the node format.
 *   t      the first segment's hit distance, with the bits of moptix_hit.t of MOPTIX_QUERY_CLOSEST on the same ray (tmax on a miss): the
 *          distance to what the radiance came from first, e.g. to place a probe's sample or to weight a texel, without a second query.
 *   An invalid ray: r = g = b = 0, t = the given tmax; no path is traced for it.
 * Nodes: the 64-byte form where the tree has one, else the 128-byte one; option "node_format" 64 / 128 forces either (same bits).
 *   moptix_query_radiance_device  dRays, dOut: device memory, 16-byte aligned; dStates: device memory, 4-byte aligned; seeds: host
 *                                 memory.  Asynchronous on the context's stream: moptix_sync, or the stream's own synchronisation,
 *                                 waits for it.  The per-sample scratch ("radiance_buffer_mb") is allocated at first use and kept;
 *                                 the stack overflow area lives in the context until moptix_clear_scene, moptix_build_accel or
 *                                 moptix_destroy.  The scene tables are read as they are when the kernel runs.
 *   moptix_query_radiance         host pointers, blocking: upload, query, read back (staging kept in the context)
 * n may be any int64 >= 0; n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or misaligned pointers, n < 0, nSamples < 1, both or neither
 * of seeds and states, unknown flag bits; state errors as moptix_query_rays ("faces dirty" before a refit included).  A radiance
 * query changes nothing else in the context: not the accumulation buffer, the depth history, the node-format verdict,
 * moptix_kernel_time, the AOV, denoiser, temporal or adaptive state, nor the ray queries' buffers. */
enum { MOPTIX_RADIANCE_CLAMP = 1 };
int moptix_query_radiance_device(moptix_context ctx, const float* dRays, int64_t n, const int32_t* seeds, const uint32_t* dStates,
                                 int32_t nSamples, uint32_t indexBase, uint32_t flags, float* dOut);
int moptix_query_radiance(moptix_context ctx, const float* rays, int64_t n, const int32_t* seeds, const uint32_t* states,
                          int32_t nSamples, uint32_t indexBase, uint32_t flags, float* out);

/* ---- point queries: the nearest surface point for the caller's own points ------------------------------------------------------------
 * What is the nearest point of the scene's surface to q, and how far is it: contact and collision, sampling a distance field,
 * closest-point correspondences, proximity masks -- on the tree the rays walk, refitted with it.
 * A query is four floats  x y z maxDist, read as one 16-byte load.  r2 = maxDist * maxDist, one binary32 multiply; maxDist = +inf is
 * allowed and means "no limit".  Needs moptix_set_params and moptix_build_accel like a ray query; the camera and the frame size play no part.
 * Per primitive there is a function d2(q, primitive): the squared distance from q to the nearest point c of the primitive, in binary32
 * under the arithmetic contract of csrc/pt_math.h (AC1-AC5, no contraction, correctly rounded division and square root).  It depends on
 * q and the primitive's device record alone; csrc/pt_point.h states every operation in order.  d2 = dot(q - c, q - c) throughout.
 *   segment (a, ab)  den = dot(ab, ab); t = clamp(dot(q - a, ab) / den, 0, 1), t = 0 when den is 0; c = a + ab * t.  Here and for the
 *              quad, clamp(x, 0, 1) is x > 0 ? (x < 1 ? x : 1) : 0 by comparisons: -0 and NaN give +0
 *   triangle   the triangle of the device record, v0 = p0, v1 = p0 + e0, v2 = p0 - e1 (e0 = p1 - p0 and e1 = p0 - p2 as stored: the
 *              triangle the ray test sees).  The minimum of up to four candidates, the first of equal ones: the segments (v0, e0),
 *              (v0, -e1), (v1, v2 - v1), and the plane projection c = (v0 + bu * e0) + bv * (-e1) with bu, bv the barycentrics of step 2 of
 *              moptix_denoise_temporal (e1 = e0, e2 = -e1 of the record, w = q - v0, unclamped) evaluated with the normal scaled by a
 *              power of two so that its largest component lies in [1, 2) -- dot(n, n) itself leaves binary32 for edges beyond 4e9 or
 *              below 1e-10 units.  The projection applies when the normal is non-zero and finite and
 *              bu >= 0, bv >= 0, bu + bv <= 1.  A zero-area triangle is thereby well defined: collinear vertices count as the longest of
 *              the three segments, coincident vertices as a point, and no NaN comes out of finite input.
 *   sphere     the surface: c = centre + radius * normalize(q - centre), with the direction (1, 0, 0) when q is the centre
 *   quad       the rectangle in the ray test's own parametrisation: a1 = clamp(dot(v1, q - anchor), 0, 1), a2 = clamp(dot(v2, q - anchor),
 *              0, 1), c = (anchor + a1 * E1) + a2 * E2 with E1 = v1 / dot(v1, v1), E2 = v2 / dot(v2, v2), the edges moptix_quad_params holds
 *              inverted
 * MOPTIX_POINT_CLOSEST -> one moptix_point_hit (32 bytes) per query: the primitive least by (d2, prim) among those with d2 < r2; at
 * exactly equal d2 the lower prim wins (rule D5).  The answer is a function of the per-primitive d2 alone -- what a loop over every
 * primitive gives, bit for bit: tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part.  Every primitive
 * counts, whatever its material.
 *   dist  sqrt(d2) of the winner, one correctly rounded square root
 *   prim  primitive id in the ray queries' numbering: spheres, then quads, then triangles by original face id; -1 = miss
 *   mat   material id of the primitive; -1 on a miss
 *   u, v  triangles: the weights of the face's second and third vertex, c = p0 + u (p1 - p0) + v (p2 - p0) up to rounding; quads: a1, a2;
 *         spheres: 0
 *   p     the nearest point c
 *   miss  dist = the given maxDist, prim = mat = -1, every other field 0
 * MOPTIX_POINT_ANY -> one int32 per query: 1 if and only if the closest mode on the same query reports prim >= 0, else 0; the walk stops
 * at the first primitive it accepts.
 * Invalid queries are misses, decided before any traversal: x, y or z non-finite, maxDist NaN, or maxDist <= 0.
 * MOPTIX_POINT_SIGNED -> one moptix_point_hit per query: every field has the bits of MOPTIX_POINT_CLOSEST on the same query, except that
 * dist is negated when q is inside.  A miss and an invalid query are exactly as in the closest mode (dist = +maxDist); maxDist limits the
 * unsigned distance.  The sign is decided from the winner's own record and its row of the sign table (csrc/pt_sign.h states every
 * operation in order), so the signed answer too is what a loop over every primitive gives, bit for bit.  With c the reported nearest
 * point:  s = dot(q - c, N),  dist = s < 0 ? -sqrt(d2) : +sqrt(d2): s == 0 (q == c included) and NaN give +.
 *   triangle   N = the angle-weighted pseudonormal (Baerentzen and Aanaes) of the feature c lies on.  The feature is DEFINED by which of
 *              the four candidates above won (the first of equal ones) and by the segment's clamped parameter t:
 *                1  segment(v0, e0)       t == 0 vertex 0, t == 1 vertex 1, else edge 01
 *                2  segment(v0, -e1)      t == 0 vertex 0, t == 1 vertex 2, else edge 02
 *                3  segment(v1, v2 - v1)  t == 0 vertex 1, t == 1 vertex 2, else edge 12
 *                4  the projection        the face
 *              not by the reported (u, v): (1 - t) + t is not always 1.
 *   sphere     inside if and only if dot(w, w) < radius * radius, w = q - centre
 *   quad       always +: a quad is an open surface
 * Topology.  Taken once per set of uploaded faces, at the first signed query or the first moptix_get_sign_info after the faces were
 * added, on the host, from the face positions of the staging (pending device-side updates are fetched back first, as moptix_build_accel
 * does).  Kept across moptix_update_faces*, moptix_refit_accel and moptix_build_accel; dropped by moptix_clear_scene, moptix_add_mesh and
 * moptix_destroy.  Corners are welded when their three position words are equal, -0 taken as +0; welded ids run in order of first
 * appearance by (face, corner); an edge is an unordered pair of welded ids.  A face with two corners welded together, or whose normal is
 * zero or non-finite, is DEGENERATE: it contributes to no sum and no count, and its record is zero (a query it wins is +).
 * Pseudonormals (not normalised: only the sign of s is used), in binary32, every operation in csrc/pt_sign.h:
 *   face    un = the unit normal of cross(p1 - p0, p2 - p0), the cross product scaled by a power of two first (as the projection above)
 *   edge    the sum of un over the edge's faces in ascending face id, from +0 by plain adds
 *   vertex  the sum over its corners in ascending (face id, corner) of un * angle, from +0 by plain adds; angle = atan2_ac(length(cross(a,
 *           b)), dot(a, b)) of the corner's two edge vectors, atan2_ac one specified binary32 algorithm (absolute error <= 1e-6)
 * Ordered sums, no float atomics: the words depend on positions and topology alone.  The stated range is edges whose cross products stay
 * finite and normal in binary32 (lengths between about 1e-9 and 1e9 units).  The table holds 96 bytes per original face id (six
 * pseudonormals v0 v1 v2 e01 e02 e12, the unit face normal, padding) and is computed on the device from the faces' current positions.  It
 * is stale after moptix_update_faces*, moptix_refit_accel and moptix_build_accel; the next signed query enqueues its build in front of the
 * query kernel on the context's stream, without a host synchronisation and without an allocation after the first.
 *   moptix_get_sign_info   works from the moment faces are uploaded and needs no built tree (zeros without faces):
 *     weldedVerts, edges   of the topology (degenerate faces add vertices, not edges)
 *     boundaryEdges        edges with one face
 *     nonManifoldEdges     edges with more than two faces
 *     flippedEdges         edges whose two faces run along them in the same direction
 *     degenerateFaces      as defined above, on the positions the topology was taken from
 *     closed               1 if and only if the previous four are 0 and there is at least one face
 *     signedVolume         sum of dot(p0, cross(p1, p2)) / 6 in binary64 over those positions; NEGATIVE means the mesh is wound inwards
 *                          and every sign comes out flipped
 *     tableBuilds          how many times the device table has been computed on this topology
 *   On a mesh that is not closed the sign is still the formula's, and is meaningless near the holes: the library reports and does not
 *   refuse.  Meshes uploaded by separate moptix_add_mesh calls weld like one.  Interpenetrating solids are not united.
 *   moptix_debug_read_sign_table   a test aid, not an interface to build on: the table (computed first if stale, which counts as a build)
 *                          copied to the host, 96 bytes per face; state errors as a query.
 * Nodes: the 64-byte form where the tree has one, else the 128-byte one; option "node_format" 64 / 128 forces either (same bits: the
 * 64-byte boxes contain the 128-byte ones, so the walk enters more boxes and finds the same minimum).
 *   moptix_query_points_device  dPoints, dOut: device memory, 16-byte aligned (dOut of MOPTIX_POINT_ANY: 4).  Asynchronous on the
 *                               context's stream: moptix_sync, or the stream's own synchronisation, waits for it.  Allocates nothing
 *                               after the first point query on a tree: the point queries keep a stack overflow area of their own,
 *                               kept across refits, until moptix_clear_scene, moptix_build_accel or moptix_destroy.  The sphere and quad
 *                               tables are read as they are when the kernel runs: a query after moptix_update_spheres sees the moved spheres.
 *   moptix_query_points         host pointers, blocking: upload, query, read back (staging kept in the context)
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 points); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_rays ("faces dirty" before a refit included).  A point query
 * changes nothing else in the context, and in particular not the ray queries' buffers; moptix_debug_buffer_addresses keeps its slots.
 * A signed query shares the point queries' stack overflow area and keeps its topology and table beside it.
 *   moptix_query_points_signed  the host-pointer, blocking form of MOPTIX_POINT_SIGNED (staging as moptix_query_points').  The mode is taken
 *                               by moptix_query_points_device; moptix_query_points itself keeps the two modes it had, and 2 stays
 *                               MOPTIX_ERR_INVALID there: nothing a caller of it relied on has changed. */
typedef struct { float dist; int32_t prim; int32_t mat; float u, v; float p[3]; } moptix_point_hit;
enum { MOPTIX_POINT_CLOSEST = 0, MOPTIX_POINT_ANY = 1, MOPTIX_POINT_SIGNED = 2 };
typedef struct {
  uint32_t weldedVerts, edges, boundaryEdges, nonManifoldEdges, flippedEdges, degenerateFaces, closed, tableBuilds;
  double signedVolume;
} moptix_sign_info;
int moptix_query_points_device(moptix_context ctx, const float* dPoints, int64_t n, int32_t mode, void* dOut);
int moptix_query_points(moptix_context ctx, const float* points, int64_t n, int32_t mode, void* out);
int moptix_query_points_signed(moptix_context ctx, const float* points, int64_t n, moptix_point_hit* out);
int moptix_get_sign_info(moptix_context ctx, moptix_sign_info* out);
int moptix_debug_read_sign_table(moptix_context ctx, void* table);

/* ---- K-nearest point queries: the maxNear nearest primitives to each point, in order --------------------------------------------------
 * Every face within a contact margin, the K best candidates of a correspondence (so that a wrong nearest triangle on a fold can be
 * rejected), "how many primitives are within r" -- in one walk, and right at exactly equal distances (duplicated faces, shared vertices),
 * where no re-launch of the closest query with another maxDist finds the second of two.
 * A query is the point queries' four floats  x y z maxDist, valid or invalid by their rule; r2 = maxDist * maxDist, +inf = no limit.
 * The near set S of a valid query is the set of pairs (d2(q, primitive), prim) over every primitive record with d2 < r2, d2 the
 * per-primitive function of the point queries: one pair per primitive, a sphere included.  Every primitive counts, whatever its material.
 * An invalid query has S = {}.  S is a function of the query and the device records alone.
 *   hits    n x maxNear moptix_point_hit records, query-major.  For query i the first c = min(maxNear, |S|) records are the c least
 *           elements of S by (d2, prim) ascending (rule D5's order), each filled exactly as MOPTIX_POINT_CLOSEST fills its record when that
 *           primitive wins: dist one correctly rounded sqrt(d2); prim, mat, u, v, p as that mode sets them.  Records c .. maxNear - 1 are
 *           that mode's miss record on the query (dist = the given maxDist's bits, prim = mat = -1, the rest 0).  Every byte is defined.
 *           Record 0 has the bits of MOPTIX_POINT_CLOSEST on the same query.
 *   counts  n x int32: c.  With MOPTIX_POINT_MULTI_COUNT_ALL: |S|, the number of primitives within maxDist -- the walk then cannot prune
 *           at the maxNear-th key, only at r2.  counts[i] > 0 if and only if MOPTIX_POINT_ANY gives 1 on the same query.
 *   maxNear 1..64.  With MOPTIX_POINT_MULTI_COUNT_ALL also 0, and hits may then be NULL: the pure in-range count.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part, and unlike the ray side there is no grazing
 * exception: the point walk's prune is proven against the padded boxes, and csrc/pt_pointmulti.h states why the proof covers the
 * maxNear-th bound.
 *   moptix_query_points_multi_device  dPoints, dHits: device memory, 16-byte aligned; dCounts: device memory, 4-byte aligned.
 *                                     Asynchronous on the context's stream.  While a point is walked its slice of dHits holds the
 *                                     candidates; nothing else is allocated or written.  It uses the point queries' stack overflow area
 *                                     (same grid cap and stack bound; allocated at the first point query of either kind on a tree).
 *   moptix_query_points_multi         host pointers, blocking: upload, query, read back (the point queries' staging)
 * n may be any int64 >= 0: longer batches are cut into launches of floor(2^30 / max(maxNear, 1)) queries, so that a launch writes at most
 * 2^30 records and a record's index within it fits an int as a point's does; n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or misaligned
 * pointers, n < 0, maxNear out of range, unknown flag bits; state errors as moptix_query_points ("faces dirty" before a refit included).
 * A K-nearest query changes nothing else in the context: moptix_debug_buffer_addresses keeps its slots, and the ray queries' buffers are
 * untouched.  Not offered: a signed list (the sign of a non-nearest primitive's pseudonormal says nothing about inside or outside),
 * filters by primitive kind or material, lists longer than 64. */
enum { MOPTIX_POINT_MULTI_COUNT_ALL = 1 };
int moptix_query_points_multi_device(moptix_context ctx, const float* dPoints, int64_t n, int32_t maxNear, uint32_t flags,
                                     void* dHits, int32_t* dCounts);
int moptix_query_points_multi(moptix_context ctx, const float* points, int64_t n, int32_t maxNear, uint32_t flags,
                              moptix_point_hit* hits, int32_t* counts);

/* ---- box queries: the primitives that meet each of the caller's axis-aligned boxes ---------------------------------------------------
 * The range question neither the rays nor the points answer (a point query with maxDist tests a ball): voxelising a mesh into an
 * occupancy grid, a broad phase that returns candidate faces per cell, box selection of faces, culling a region before a costlier
 * query -- on the tree the rays walk, refitted with it.
 * A box is six floats  lox loy loz hix hiy hiz.  Valid: all six finite and lo <= hi on every axis; lo == hi is allowed, so a box may be
 * a point, a segment or a rectangle.  An invalid box overlaps nothing, decided before any traversal.
 * Boxes and primitives are closed sets: touching counts.  All arithmetic is binary32 under the contract of csrc/pt_math.h, without
 * contraction; csrc/pt_box.h states every operation in order.  S(box) is the set of primitive ids whose predicate holds; ids are the
 * queries' (spheres, then quads, then triangles by original face id); every primitive counts, whatever its material.  S is a function of
 * the box and the device records alone.
 *   triangle   the record's triangle as the point queries see it (v0 = p0, v1 = p0 + e0, v2 = p0 - e1), by the 13-axis separating-axis
 *              test in three steps, any of which may reject: (A) the per-axis min / max of the computed vertices against lo / hi, exact
 *              comparisons; (B) with c = lo * 0.5 + hi * 0.5, h = hi * 0.5 - lo * 0.5, u_i = v_i - c and the edges f0 = u1 - u0,
 *              f1 = u2 - u1, f2 = u0 - u2, the nine axes a = cross(e_k, f_j), each as its two-term expression: p_i = dot(a, u_i) over the
 *              non-zero terms, r = h . |a|, reject if min p > r or max p < -r; (C) n = cross(f0, f1), d = dot(n, u0), r = dot(h, |n|),
 *              reject if |d| > r.  Rejections are strict, so a NaN or an equality rejects nothing; a zero-area triangle needs no special
 *              case.
 *   sphere     the surface: dmin2 = the squared distance from the centre to the box, dmax2 = the sum over the axes of
 *              max(|c - lo|, |hi - c|)^2, r2 = radius * radius; overlap iff dmin2 <= r2 and dmax2 >= r2.  A box wholly inside the ball
 *              meets nothing.
 *   quad       the four corners (anchor + E1 * a1) + E2 * a2 at a in {0, 1} of the point queries' parametrisation; the triangles
 *              (c00, c10, c11) and (c00, c11, c01) through the triangle predicate; the quad overlaps if either does.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part, and there is no grazing exception: the walk
 * enters a child iff its box and the query box overlap by exact comparisons, and csrc/pt_box.h proves from the builder's padding that this
 * loses no primitive of S.
 *   MOPTIX_BOX_ANY    one int32 per box: |S| > 0.  The walk stops at the first primitive accepted.
 *   MOPTIX_BOX_COUNT  one int32 per box: |S|.
 *   list              offsets: n + 1 int64 entries, non-decreasing, into prims (int32): the capacity of box i is
 *                     offsets[i + 1] - offsets[i]; a negative capacity reads as 0.  counts[i] = |S| always.  If |S| <= capacity the slice
 *                     holds S in ascending id, then -1 up to the capacity; otherwise the whole slice is -1 and the caller sees
 *                     counts[i] > capacity.  Every byte of every slice is defined and nothing of the answer depends on the tree; the K
 *                     lowest ids of a longer set are deliberately not offered.  The ids are appended to the box's own slice while they
 *                     fit and sorted there in place: nothing else is allocated.
 *   moptix_query_boxes_device       dBoxes: device memory, 8-byte aligned (a box is read as three 8-byte loads); dOut: device memory,
 *                                   4-byte aligned.  Asynchronous on the context's stream.
 *   moptix_query_boxes              host pointers, blocking: upload, query, read back (staging kept in the context)
 *   moptix_query_boxes_list_device  dBoxes, dOffsets: 8-byte aligned; dPrims, dCounts: 4-byte aligned.  Asynchronous.  The offsets are
 *                                   the caller's to get right: the kernel writes where they point.
 *   moptix_query_boxes_list         host pointers, blocking; offsets are checked here: non-decreasing, offsets[0] >= 0.  prims is
 *                                   written from offsets[0] to offsets[n].
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 boxes); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_points ("faces dirty" before a refit included).
 * The box queries keep a stack overflow area of their own, sized like the others' by the tree's stack bound, the grid cap and
 * "query_blocks_per_cu": allocated at the first box query on a tree, kept across refits, dropped by moptix_clear_scene, moptix_build_accel
 * and moptix_destroy.  A box query changes nothing else in the context: moptix_debug_buffer_addresses keeps its slots, and the ray and
 * point queries' buffers are untouched.  Sphere and quad tables are read as they are when the kernel runs (moptix_update_spheres).
 * Not offered: filters by material or primitive kind (oriented boxes, frusta and query triangles: the next three sections). */
enum { MOPTIX_BOX_ANY = 0, MOPTIX_BOX_COUNT = 1 };
int moptix_query_boxes_device(moptix_context ctx, const float* dBoxes, int64_t n, int32_t mode, int32_t* dOut);
int moptix_query_boxes(moptix_context ctx, const float* boxes, int64_t n, int32_t mode, int32_t* out);
int moptix_query_boxes_list_device(moptix_context ctx, const float* dBoxes, int64_t n, const int64_t* dOffsets, int32_t* dPrims,
                                   int32_t* dCounts);
int moptix_query_boxes_list(moptix_context ctx, const float* boxes, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts);

/* ---- oriented box queries: the primitives that meet each of the caller's rotated boxes -------------------------------------------------
 * The box queries' question for a box with axes of its own: the broad phase of rigid bodies against a mesh that is refitted every step (a
 * long body on a diagonal has a world box many times its own), selection of faces in a tilted region, candidate faces for a swept or
 * rotated tool, culling a slab or a beam before a costlier query.
 * A box is sixteen floats, 64 bytes:  cx cy cz  hx hy hz  a0.x a0.y a0.z  a1.x a1.y a1.z  a2.x a2.y a2.z  and one float that is not read:
 * the centre, the half-extents along the box's own axes, and those axes as world-space directions (the columns of the usual
 * local-to-world rotation).  The box is the closed set { x : |dot(a_j, x - c)| <= h_j, j = 0, 1, 2 }.  Valid: floats 0..14 finite; h_j >= 0
 * (h_j == 0 is allowed, so a box may be a rectangle, a segment or a point); the axes orthonormal within 2^-10, |dot(a_i, a_i) - 1| <= 2^-10
 * and |dot(a_i, a_j)| <= 2^-10 for i < j, in binary32.  An invalid box meets nothing, decided before any traversal.
 * Touching counts.  All arithmetic is binary32 under the contract of csrc/pt_math.h, without contraction; csrc/pt_obb.h states every
 * operation in order.  S(obb) is the set of primitive ids whose predicate holds; ids are the box queries' (spheres, then quads, then
 * triangles by original face id); every primitive counts.  S is a function of the sixteen floats and the device records alone.
 *   triangle   the record's triangle as the box queries see it.  (W) the per-axis min / max of the computed vertices against the query's
 *              grown world box c -+ (E + g_w), E_k = (|a0.k| h0 + |a1.k| h1) + |a2.k| h2, g_w = max h * 2^-6 + (max |c| + max h) * 2^-16,
 *              exact comparisons, strict rejections; (L) u_i = (dot(a_j, v_i - c))_j, then the box queries' triangle predicate on u_0, u_1,
 *              u_2 against the box -h .. +h, unchanged.  W is there so that the walk's world-axis test is part of the predicate; g_w is
 *              chosen so that it rejects nothing L accepts (csrc/pt_obb.h).
 *   sphere     the surface: m = (dot(a_j, centre - c))_j, then the box queries' sphere predicate on m and -h .. +h.  A box wholly inside
 *              the ball meets nothing.  Exact up to the axes' departure from orthonormality.
 *   quad       the four corners of the box queries' quad as two triangles through the triangle predicate.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part: the walk enters a child iff its box meets the
 * grown world box by exact comparisons and passes a six-axis test against the box's own axes with a margin, and csrc/pt_obb.h proves
 * from the builder's padding and a bound on the roundings that this loses no primitive of S, in both node forms and after a refit.
 *   mode       MOPTIX_BOX_ANY / MOPTIX_BOX_COUNT as for moptix_query_boxes.
 *   list       the box queries' contract, word for word: offsets are n + 1 non-decreasing int64 entries into prims; counts[i] = |S|
 *              always; if |S| <= capacity the slice holds S in ascending id, then -1 up to the capacity; otherwise the whole slice is -1
 *              and the caller sees counts[i] > capacity.  Every byte of every slice is defined.
 *   moptix_query_obbs_device       dObbs: device memory, 16-byte aligned (a box is read as four 16-byte loads); dOut: device memory,
 *                                  4-byte aligned.  Asynchronous on the context's stream: no host wait, no allocation on a warm call.
 *   moptix_query_obbs              host pointers, blocking: upload, query, read back (staging kept in the context)
 *   moptix_query_obbs_list_device  dObbs: 16-byte aligned; dOffsets: 8-byte aligned; dPrims, dCounts: 4-byte aligned.  Asynchronous.  The
 *                                  offsets are the caller's to get right: the kernel writes where they point.
 *   moptix_query_obbs_list         host pointers, blocking; offsets are checked here: non-decreasing, offsets[0] >= 0.
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 boxes); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_boxes ("faces dirty" before a refit included).
 * The oriented box queries keep a stack overflow area of their own: allocated at the first such query on a tree, kept across refits,
 * dropped by moptix_clear_scene, moptix_build_accel and moptix_destroy.  They change nothing else in the context:
 * moptix_debug_buffer_addresses keeps its slots, and the other queries' buffers are untouched.
 * Not offered: sheared boxes (axes that are not orthonormal; up to six planes of any kind: the frustum queries), exact plane sharing between neighbouring
 * oriented cells (two cells' faces are each rounded in their own frame; moptix_query_boxes' grids share planes exactly), filters by
 * material or primitive kind. */
int moptix_query_obbs_device(moptix_context ctx, const float* dObbs, int64_t n, int32_t mode, int32_t* dOut);
int moptix_query_obbs(moptix_context ctx, const float* obbs, int64_t n, int32_t mode, int32_t* out);
int moptix_query_obbs_list_device(moptix_context ctx, const float* dObbs, int64_t n, const int64_t* dOffsets, int32_t* dPrims,
                                  int32_t* dCounts);
int moptix_query_obbs_list(moptix_context ctx, const float* obbs, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts);

/* ---- frustum queries: the primitives that meet each of the caller's six-plane regions ----------------------------------------------------
 * The box queries' question for a convex region bounded by planes: which faces a camera or a screen tile can see (view culling, marquee
 * selection of faces, per-tile candidate lists), which faces lie in a portal, a wedge, a slab, a half-space or a k-DOP of up to six planes.
 * A query is 24 floats, 96 bytes: six planes  nx ny nz d.  The region is the closed set { x : dot(n_j, x) + d_j >= 0, j = 0..5 }: normals
 * point inwards (what Gribb-Hartmann extraction from a clip matrix gives) and need not be unit length.  Valid: all 24 floats finite.  An
 * invalid query meets nothing, decided before any traversal.  A plane 0 0 0 d with d >= 0 constrains nothing, so wedges, slabs,
 * half-spaces and unbounded pyramids need no special case; with d < 0 it empties the region; six zero planes meet every primitive.
 * Touching counts.  All arithmetic is binary32 under the contract of csrc/pt_math.h, without contraction; csrc/pt_frustum.h states every
 * operation in order.  S(frustum) is the set of primitive ids whose predicate holds; ids are the box queries' (spheres, then quads, then
 * triangles by original face id); every primitive counts.  S is a function of the 24 floats and the device records alone; it does not
 * depend on the order of the six planes, nor on a plane's four floats being multiplied by a power of two (short of overflow and underflow).
 *   triangle   the record's triangle as the box queries see it, s_ji = dot(n_j, v_i) + d_j.  (R) reject if on some plane all three
 *              s_ji < 0; (A) accept if some vertex has s_ji >= 0 on all six; (E) clip each edge as a parameter interval against the six
 *              planes, t = s_a / (s_a - s_b), accept if one is left non-empty; (V) for a face that cuts through the region with all
 *              edges outside: the crossings of the 15 pairs of plane lines in the triangle's own coordinates, accept if one lies in the
 *              triangle and on the inner side of the other four planes.  An exact stage behind the plane test: a triangle outside no
 *              single plane and still outside the region is not reported.
 *   sphere     the plane rule on the BALL: s_j = dot(n_j, centre) + d_j >= -(radius * |n_j|) on all six planes, |n_j| = sqrtf(dot(n_j,
 *              n_j)) taken once per query.  What view culling asks ("can the ball be seen"); exact for half-spaces and slabs.  Not the
 *              surface the box queries test: a region wholly inside the ball meets it.  Conservative at the region's edges and
 *              corners: a ball within `radius` of two planes but not of their common edge is reported.  Two contradictory planes still
 *              report a ball that reaches across both; a plane 0 0 0 d with d < 0 reports nothing.
 *   quad       the four corners of the box queries' quad as two triangles through the triangle predicate.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part: the walk enters a child iff the largest value
 * of each plane's function over the child's box is at least minus a margin of 2^-16 of the magnitudes involved, and csrc/pt_frustum.h
 * proves from the builder's padding and a bound on the roundings (the margin is sixteen times it) that this loses no primitive of S, in
 * both node forms and after a refit.
 *   mode       MOPTIX_BOX_ANY / MOPTIX_BOX_COUNT as for moptix_query_boxes.
 *   list       the box queries' contract, word for word: offsets are n + 1 non-decreasing int64 entries into prims; counts[i] = |S|
 *              always; if |S| <= capacity the slice holds S in ascending id, then -1 up to the capacity; otherwise the whole slice is -1
 *              and the caller sees counts[i] > capacity.  Every byte of every slice is defined.
 *   moptix_query_frusta_device       dFrusta: device memory, 16-byte aligned (a query is read as six 16-byte loads); dOut: device memory,
 *                                    4-byte aligned.  Asynchronous on the context's stream: no host wait, no allocation on a warm call.
 *   moptix_query_frusta              host pointers, blocking: upload, query, read back (staging kept in the context)
 *   moptix_query_frusta_list_device  dFrusta: 16-byte aligned; dOffsets: 8-byte aligned; dPrims, dCounts: 4-byte aligned.  Asynchronous.
 *                                    The offsets are the caller's to get right: the kernel writes where they point.
 *   moptix_query_frusta_list         host pointers, blocking; offsets are checked here: non-decreasing, offsets[0] >= 0.
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 queries); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_boxes ("faces dirty" before a refit included).
 * The frustum queries keep a stack overflow area of their own: allocated at the first such query on a tree, kept across refits, dropped
 * by moptix_clear_scene, moptix_build_accel and moptix_destroy.  They change nothing else in the context:
 * moptix_debug_buffer_addresses keeps its slots, and the other queries' buffers are untouched.
 * Not offered: more than six planes per query, the exact ball or the sphere's surface against the region, thin-lens frusta, filters by
 * material or primitive kind. */
int moptix_query_frusta_device(moptix_context ctx, const float* dFrusta, int64_t n, int32_t mode, int32_t* dOut);
int moptix_query_frusta(moptix_context ctx, const float* frusta, int64_t n, int32_t mode, int32_t* out);
int moptix_query_frusta_list_device(moptix_context ctx, const float* dFrusta, int64_t n, const int64_t* dOffsets, int32_t* dPrims,
                                    int32_t* dCounts);
int moptix_query_frusta_list(moptix_context ctx, const float* frusta, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts);

/* ---- triangle queries: the primitives that meet each of the caller's triangles ------------------------------------------------------------
 * The box queries' question for another triangle: the narrow phase of mesh against mesh.  The self-collision test of a mesh that
 * moptix_update_faces / moptix_refit_accel deform every step, the candidate pairs of intersection curves and booleans, a tool against a
 * part, the exact answer behind a box or oriented box broad phase.
 * A query is nine floats, 36 bytes:  ax ay az  bx by bz  cx cy cz, the three vertices -- a row of a contiguous (n, 3, 3) array
 * vertices[faces].  Valid: all nine finite.  An invalid query meets nothing, decided before any traversal.  A zero-area query (a segment,
 * a point) is valid.  Triangles are closed sets: touching counts.  All arithmetic is binary32 under the contract of csrc/pt_math.h, without
 * contraction; csrc/pt_tri.h states every operation in order.  S(query) is the set of primitive ids whose predicate holds; ids are the box
 * queries' (spheres, then quads, then triangles by original face id); every primitive counts.  S is a function of the nine floats and the
 * device records alone.
 *   triangle   the record's triangle as the box queries see it.  (A) the per-axis min / max of its computed vertices against the exact
 *              min / max box of the query's vertices, strict rejections -- the box queries' own first step; (B) both triangles in the
 *              frame at the query's first vertex (a is subtracted from all six vertices), then a separating-axis test over 23 axes in a
 *              fixed order: the two normals n1, n2; the nine cross(e_i, f_j) of the query's edges e and the primitive's f; cross(n1, e_i),
 *              cross(n1, f_j), cross(n2, e_i), cross(n2, f_j).  On each axis both triangles' three vertices are projected and the pair is
 *              rejected if one interval lies strictly beyond the other: a NaN, an equality or a zero axis rejects nothing.  The
 *              cross-normal axes decide coplanar pairs and a segment or point against a triangle of non-zero area.
 *              Two zero-area triangles against each other are decided by no finite axis list: for such a pair the predicate is still
 *              this fixed function, but only a superset of the geometric answer (it misses no pair that meets).
 *   sphere     the surface: dmin2 = the squared distance from the centre to the query triangle (the point queries' triangle function),
 *              dmax2 = the largest squared distance to a vertex; overlap iff dmin2 <= radius^2 <= dmax2.  A triangle wholly inside the
 *              ball meets nothing.
 *   quad       the four corners of the box queries' quad as two triangles through the triangle predicate.
 * Tree, leaf size, builder, node format, "query_blocks_per_cu" and scheduling play no part: the walk is the box queries' own against the
 * query's box, step A makes that test part of the predicate, and csrc/pt_tri.h carries the box queries' proof over: the answer is the loop's
 * over every primitive, with no margin, in both node forms and after a refit.
 *   mode       MOPTIX_BOX_ANY / MOPTIX_BOX_COUNT as for moptix_query_boxes.
 *   list       the box queries' contract, word for word: offsets are n + 1 non-decreasing int64 entries into prims; counts[i] = |S|
 *              always; if |S| <= capacity the slice holds S in ascending id, then -1 up to the capacity; otherwise the whole slice is -1
 *              and the caller sees counts[i] > capacity.  Every byte of every slice is defined.
 *   moptix_query_tris_device       dTris: device memory, 4-byte aligned (a query is read as nine 4-byte loads); dOut: device memory,
 *                                  4-byte aligned.  Asynchronous on the context's stream: no host wait, no allocation on a warm call.
 *   moptix_query_tris              host pointers, blocking: upload, query, read back (staging kept in the context)
 *   moptix_query_tris_list_device  dTris: 4-byte aligned; dOffsets: 8-byte aligned; dPrims, dCounts: 4-byte aligned.  Asynchronous.  The
 *                                  offsets are the caller's to get right: the kernel writes where they point.
 *   moptix_query_tris_list         host pointers, blocking; offsets are checked here: non-decreasing, offsets[0] >= 0.
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 queries); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_boxes ("faces dirty" before a refit included).
 * The triangle queries keep a stack overflow area of their own: allocated at the first such query on a tree, kept across refits, dropped
 * by moptix_clear_scene, moptix_build_accel and moptix_destroy.  They change nothing else in the context:
 * moptix_debug_buffer_addresses keeps its slots, and the other queries' buffers are untouched.
 * A query equal to a face of the mesh finds that face and its neighbours (they touch); Context.self_intersections of the Python layer
 * drops the pairs that share a vertex index.
 * Not offered: the intersection segment of a pair, signed penetration depth, time-continuous triangle-triangle contact, a device-side
 * pairing kernel, an exact answer for two zero-area triangles, filters by material or primitive kind. */
int moptix_query_tris_device(moptix_context ctx, const float* dTris, int64_t n, int32_t mode, int32_t* dOut);
int moptix_query_tris(moptix_context ctx, const float* tris, int64_t n, int32_t mode, int32_t* out);
int moptix_query_tris_list_device(moptix_context ctx, const float* dTris, int64_t n, const int64_t* dOffsets, int32_t* dPrims,
                                  int32_t* dCounts);
int moptix_query_tris_list(moptix_context ctx, const float* tris, int64_t n, const int64_t* offsets, int32_t* prims, int32_t* counts);

/* ---- winding-number queries: inside / outside for the meshes users actually have ----------------------------------------------------
 * MOPTIX_POINT_SIGNED takes its sign from pseudonormals, which is right only for a closed, consistently wound mesh.  The generalised
 * winding number w(q) (Jacobson et al. 2013) is the sum of the signed solid angles of all primitives seen from q over 4 pi: 1 inside and
 * 0 outside a closed mesh wound outwards (-1 inside one wound inwards), and a smooth function of q across holes, flipped and duplicated
 * faces; w > 0.5 classifies.  Summed over every face it costs O(faces) a point; with the order-1 far field over the tree (Barill et al.
 * 2018) O(log faces).
 * A query is 16 bytes x y z beta, the point queries' row with beta in the maxDist slot.  beta is +inf (exact: no cluster is ever
 * approximated) or finite >= 1 (2 is the usual choice; larger is more exact and slower).  A non-finite coordinate, beta < 1 or a NaN beta
 * gives the quiet NaN 0x7fc00000.  The result is one float per point.  All per-term arithmetic is binary32 under the contract of
 * csrc/pt_math.h, without contraction; the sum is binary64; csrc/pt_winding.h states every operation in order:
 *   triangle   a, b, c = the vertices minus q, scaled by the exact power of two 2^-floor(log2 of their largest |component|);
 *              det = dot(a, cross(b, c)), den = |a||b||c| + dot(a,b)|c| + dot(b,c)|a| + dot(c,a)|b|, omega = copysign(2 atan2_ac(|det|,
 *              den), det).  det == 0 gives exactly 0: a point in a face's plane gets nothing from that face.
 *   quad       the two triangles of the box queries' split; an open surface.
 *   sphere     4 pi when dot(w, w) < radius * radius, w = q - centre (the signed query's inside test), else 0.
 *   cluster    each child reference of a node carries A (sum of face areas), p (area-weighted centroid), N (sum of the area vectors
 *              1/2 cross(p1 - p0, p2 - p0)) and a radius r that is not smaller than the distance from the stored p to the farthest corner
 *              of the child's stored box.  With d = p - q, l2 = dot(d, d): the child is approximated iff l2 > (beta r)(beta r), by the
 *              dipole dot(N, d) / (l2 sqrt(l2)).
 *   sum        binary64, in a fixed order: spheres by id, quads by id, the tree depth first with children in slot order and a leaf's
 *              triangles in record order; w = (float)(sum * (1 / 4 pi)).
 * TREE DEPENDENCE.  Unlike every other query here, the value depends on the tree.  For a finite beta it does so through the
 * approximation: leaf size and builder decide which clusters exist.  For beta = +inf it depends on the tree only through the order of
 * a binary64 sum of the same binary32 terms.  The node format plays no part (references and moments are read, never a box), nor do
 * "query_blocks_per_cu" and scheduling.  Stated range: differences p - q finite; distances from q to a cluster between about 1e-12 and
 * 1e12 units (l2 sqrt(l2) finite and normal); edges between about 1e-9 and 1e9 units, as for the signed queries.
 * The moments table holds 128 bytes per node.  It is computed on the device, one launch per level of the tree, deepest first, over the
 * refit's plan, and is stale after moptix_update_faces*, moptix_refit_accel and moptix_build_accel; the next winding query enqueues the pass in
 * front of its kernel.  A context that never asks for a winding number allocates and launches nothing of this.
 *   moptix_query_winding_device  dPoints: device memory, 16-byte aligned; dOut: device memory, 4-byte aligned.  Asynchronous on the context's
 *                                stream: no host wait and no allocation on a warm call.  The first call after moptix_build_accel makes
 *                                the refit's plan where no refit has (that reads the nodes back: one host synchronisation per built tree).
 *   moptix_query_winding         host pointers, blocking: upload, query, read back (staging kept in the context)
 *   moptix_get_winding_info      tableBuilds: moments passes enqueued by this context so far; nodes: nodes of the built tree; tableBytes: bytes
 *                                of the table as allocated (0 before the first query on a tree); stale: 1 if the next query will run the pass
 *   moptix_debug_read_winding_table  a test aid, not an interface to build on: the table (computed first if stale, which counts as a build)
 *                                copied to the host, 128 bytes per node (per child slot: A, p.xyz, N.xyz, r); state errors as a query.
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 points); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0; state errors as moptix_query_points ("faces dirty" before a refit included).  An empty scene gives 0.
 * The winding queries keep a stack overflow area of their own beside the table; both are dropped by moptix_clear_scene, moptix_build_accel
 * and moptix_destroy.  They change nothing else in the context.
 * Not offered: second- and third-order expansions, a signed distance fused into the same kernel, multi-GPU splitting of the points. */
typedef struct { uint32_t tableBuilds, nodes; uint64_t tableBytes; uint32_t stale, pad; } moptix_winding_info;
int moptix_query_winding_device(moptix_context ctx, const float* dPoints, int64_t n, float* dOut);
int moptix_query_winding(moptix_context ctx, const float* points, int64_t n, float* out);
int moptix_get_winding_info(moptix_context ctx, moptix_winding_info* out);
int moptix_debug_read_winding_table(moptix_context ctx, void* table);

/* ---- sweep queries: the first contact of a moving sphere ---------------------------------------------------------------------------
 * The continuous question the rays (no radius), the points (one instant) and the boxes (no time) leave open: a sphere of radius r moves
 * from o along d; when does it first touch the scene, and where?  Continuous collision detection of particles against a mesh that is
 * refitted every step, character and camera controllers, clearance checks of a motion, thick rays.
 * A sweep is eight floats  ox oy oz dx dy dz radius tmax : the ray layout with radius in the tmin slot.  The centre is c(t) = o + d * t
 * for t in [0, tmax], in units of |d|; d is used as given.  Invalid -- a miss, decided before any traversal: a non-finite component,
 * d = 0, radius <= 0 or tmax <= 0 (a ray is the ray queries' business).
 * All arithmetic is binary32 under the contract of csrc/pt_math.h, without contraction; csrc/pt_sweep.h states every operation in order.
 * toi(prim) is the least t in [0, tmax] at which the sphere touches the primitive -- ids are the queries' (spheres, then quads, then
 * triangles by original face id); every primitive counts, whatever its material:
 *   triangle   the record's triangle as the point queries see it.  0 if the point query's d2 at o is <= radius^2, so a sweep that starts
 *              in contact reports t = 0 exactly.  Otherwise the least of up to seven candidates: the face (the plane offset by radius
 *              towards the origin's side, accepted by the point query's inside test), the three edges (ray against the cylinder, edge
 *              parameter in [0, 1]) and the three vertices (ray against the sphere), each quadratic solved about the foot of the
 *              perpendicular.  A zero-area triangle needs no special case; no NaN comes out of finite input.
 *   sphere     from outside the ray against the surface at radius R + radius; from inside t = 0 if the surface is within radius of o, else
 *              the root against R - radius where that is positive.
 *   quad       the two triangles of the box queries' corners.
 *   MOPTIX_SWEEP_CLOSEST  one moptix_sweep_hit (32 bytes) per sweep: the primitive least by (toi, prim); at exactly equal toi the lower
 *                         id.  t = toi; p, u, v are the point query's nearest point and parameters for the centre c(t) = o + d * t on
 *                         that primitive: the contact point.  The contact normal is (c(t) - p) / radius.  A miss: t = tmax as given,
 *                         prim = mat = -1, u = v = p = 0.
 *   MOPTIX_SWEEP_ANY      one int32 per sweep: 1 iff MOPTIX_SWEEP_CLOSEST reports a primitive.  The walk stops at the first contact.
 * The answer is a function of the sweep and the device records alone: tree, leaf size, builder, node format, "query_blocks_per_cu" and
 * scheduling play no part (csrc/pt_sweep.h derives the margins of the walk's prune from the builder's padding).
 *   moptix_query_sweeps_device  dSweeps: device memory, 16-byte aligned; dOut: device memory, 16-byte aligned (closest) or 4-byte aligned
 *                               (any).  Asynchronous on the context's stream.
 *   moptix_query_sweeps         host pointers, blocking: upload, query, read back (staging kept in the context)
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 sweeps); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_points ("faces dirty" before a refit included).
 * The sweep queries keep a stack overflow area of their own, sized like the others': allocated at the first sweep query on a tree, kept
 * across refits, dropped by moptix_clear_scene, moptix_build_accel and moptix_destroy.  A sweep query changes nothing else in the
 * context.  Sphere and quad tables are read as they are when the kernel runs (moptix_update_spheres).
 * Not offered: swept boxes or capsules, rotating or growing spheres, all contacts along the path, filters by material. */
enum { MOPTIX_SWEEP_CLOSEST = 0, MOPTIX_SWEEP_ANY = 1 };
typedef struct { float t; int32_t prim; int32_t mat; float u, v; float p[3]; } moptix_sweep_hit;
int moptix_query_sweeps_device(moptix_context ctx, const float* dSweeps, int64_t n, int32_t mode, void* dOut);
int moptix_query_sweeps(moptix_context ctx, const float* sweeps, int64_t n, int32_t mode, void* out);

/* ---- segment queries: the nearest surface point to each segment ---------------------------------------------------------------------
 * The question the point queries answer for a point, asked for a segment: how far is it from the scene, and where.  The edge-edge half
 * of a proximity narrow phase (moptix_query_points is the vertex-face half), clearance and contact of a capsule -- a segment with a
 * radius -- against a mesh that is refitted every step, cables, rods, tool shafts.
 * A segment is eight floats  ax ay az bx by bz maxDist pad , read as two 16-byte loads; pad is ignored.  r2 = maxDist * maxDist, +inf =
 * no limit, exactly as for the point queries.  Invalid -- a miss, decided before any traversal: any of the six coordinates non-finite,
 * maxDist NaN or maxDist <= 0.  a == b is valid: against a triangle or a sphere it is the point query's function, so in a scene without
 * quads the record's dist, prim, mat and p are the point query's bit for bit.  A quad is measured as its two triangles here and by its
 * clamped coordinates there: in a scene with quads the two queries can name different primitives for the same point.
 * All arithmetic is binary32 under the contract of csrc/pt_math.h, without contraction; csrc/pt_segment.h states every operation in order.
 * d2(prim) -- ids are the queries' (spheres, then quads, then triangles by original face id); every primitive counts, whatever its material:
 *   triangle   the record's triangle as the point queries see it.  The least of six candidates, the first of equal ones: the point query's
 *              answer at a (feature 0, s = 0) and at b (1, s = 1); the closest pair between the segment and each edge, in the point query's
 *              edge order (2, 3, 4), by one segment-segment routine that is clamps and comparisons only; and the crossing (5): the ray
 *              queries' own triangle test on (a, b - a) over (0, 1) accepts at t, then d2 = 0, s = t, p = a + (b - a) * t.  "Distance 0" is
 *              "the closest ray query on that ray can report this triangle".  A zero-area triangle needs no special case; no NaN comes
 *              out of finite input.
 *   sphere     the surface.  With dmin the centre's distance to the segment and dmax the larger of the ends' distances to it:
 *              dmin > R: dmin - R, at the segment's point nearest the centre (feature 0 or 1 at an end, 2 in between); dmax < R: R - dmax,
 *              at that end (0 or 1); otherwise 0, at the first point of the segment on the surface (5).
 *   quad       the two triangles of the box queries' corners; the second triangle's edges report feature 6, 7, 8.
 *   MOPTIX_SEGMENT_CLOSEST  one moptix_segment_hit (32 bytes, two 16-byte stores) per segment: the primitive least by (d2, prim) among
 *                           those with d2 < r2; at exactly equal d2 the lower id.  dist = sqrt(d2); s in [0, 1] the parameter of the
 *                           nearest point a + (b - a) * s on the segment; p the nearest point on the primitive; feature the candidate
 *                           that won.  A miss: dist = maxDist as given, prim = mat = -1, s = p = feature = 0.
 *   MOPTIX_SEGMENT_ANY      one int32 per segment: 1 iff MOPTIX_SEGMENT_CLOSEST reports a primitive.  The walk stops at the first
 *                           primitive it accepts.
 * The answer is a function of the segment and the device records alone: tree, leaf size, builder, node format, "query_blocks_per_cu" and
 * scheduling play no part (csrc/pt_segment.h derives the margin of the walk's prune).
 *   moptix_query_segments_device  dSegments: device memory, 16-byte aligned; dOut: device memory, 16-byte aligned (closest) or 4-byte
 *                                 aligned (any).  Asynchronous on the context's stream.
 *   moptix_query_segments         host pointers, blocking: upload, query, read back (staging kept in the context)
 * n may be any int64 >= 0 (longer batches are cut into launches of 2^30 segments); n == 0 -> MOPTIX_OK.  MOPTIX_ERR_INVALID: null or
 * misaligned pointers, n < 0, an unknown mode; state errors as moptix_query_points ("faces dirty" before a refit included).
 * The segment queries keep a stack overflow area of their own, sized like the others': allocated at the first segment query on a tree,
 * kept across refits, dropped by moptix_clear_scene, moptix_build_accel and moptix_destroy.  A segment query changes nothing else in the
 * context.  Sphere and quad tables are read as they are when the kernel runs (moptix_update_spheres).
 * WARNING, segments in a primitive's plane.  "Distance 0" is the ray queries' triangle test, which is exact to
 * nu / sin(angle between the segment and the plane), nu = 2^-19 (|b - a| + the largest |vertex - a|), for a segment that comes within nu
 * of the plane, and undefined for a segment IN the plane: such a segment can be reported as crossing (dist = 0, feature = 5) a triangle
 * or quad of that plane that lies beside it, at any distance, and there the answer may depend on the tree.  Edges of a flat region
 * queried against the region's own non-incident faces are this case (edge_proximity on a planar patch): lift them off the plane by more
 * than nu, or ignore feature 5 on faces coplanar with the edge.  Every other feature is a distance, good to 1e-7 of the scene's extent.
 * Not offered: a radius per segment (subtract it from dist; it belongs in maxDist), all primitives within maxDist, swept capsules. */
enum { MOPTIX_SEGMENT_CLOSEST = 0, MOPTIX_SEGMENT_ANY = 1 };
typedef struct { float dist; int32_t prim; int32_t mat; float s; float p[3]; int32_t feature; } moptix_segment_hit;
int moptix_query_segments_device(moptix_context ctx, const float* dSegments, int64_t n, int32_t mode, void* dOut);
int moptix_query_segments(moptix_context ctx, const float* segments, int64_t n, int32_t mode, void* out);

/* ---- mesh updates and refit ------------------------------------------------- */
/* Moves the vertices of uploaded faces and fits the built tree to them in place, without a rebuild.
 * Faces are numbered in upload order across all moptix_add_mesh calls: the prim a triangle reports (moptix_hit, the AOVs' primId)
 * minus the numbers of spheres and quads.  The face count and which vertices a face joins cannot change: that takes moptix_clear_scene.
 *   moptix_update_faces         pos9: 9 floats per face, p0 p1 p2 (from indexed data: verts[faces]); nrm9: NULL = the normals stay, else 9
 *                               floats per face, stored only for faces that had normals at upload (which faces have normals does not
 *                               change).  Materials, texcoords and shadow classes stay.  Host memory; copied before the call returns.
 *   moptix_update_faces_device  the same from device memory (4-byte aligned), as device-to-device copies enqueued on the context's stream:
 *                               the caller's buffers must stay valid, and their contents ready, until the stream has run them
 *                               (moptix_sync).  The values are not inspected.  A later moptix_build_accel first fetches them back into
 *                               the host staging.  Before moptix_build_accel there is no device copy to write: the call then blocks
 *                               and copies into the host staging.
 * MOPTIX_ERR_INVALID: firstFace < 0, nFaces < 0, a range past the last face, null positions (with nFaces > 0), a misaligned device
 * pointer, a non-finite value (host form).  nFaces == 0 changes nothing.
 * Before moptix_build_accel an update only edits the staging.  On a built scene it leaves the context "faces dirty": the tree no
 * longer bounds the triangles, so every entry point that traces (moptix_launch / render*, moptix_render_aovs, moptix_render_adaptive,
 * moptix_query_rays*, moptix_query_radiance*, moptix_query_points*, moptix_query_boxes*, moptix_query_obbs*, moptix_query_frusta*, moptix_query_tris*, moptix_query_winding*, moptix_query_sweeps*, moptix_query_segments*, moptix_debug_trace, moptix_validate) returns MOPTIX_ERR_STATE until moptix_refit_accel or moptix_build_accel has
 * run.  The denoiser entries do not trace and are not affected.
 *   moptix_refit_accel          blocking, on the context's stream.  Keeps the tree's topology and the order of the triangle records and
 *                               rewrites every triangle record (p0, e0 = p1 - p0, e1 = p0 - p2; material, face id and shadow class
 *                               kept), every shading record, every child box of every 128-byte node and every 64-byte node:
 *                                 scene box     min / max over the faces' boxes; padAbs = 1e-5 * its largest extent + 1e-30
 *                                 triangle      its box from the three positions, padded as the builder pads (by padAbs + 1e-6 |v|)
 *                                 leaf child    min / max over its triangles' padded boxes
 *                                 node child    min / max over the child boxes of that node
 *                                 64-byte node  the builder's compression of the 128-byte node
 *                               Unused child slots, references and counts are untouched.  min / max are exact, so the result does not
 *                               depend on scheduling, and a refit over unchanged positions reproduces the built tree word for word.
 *                               If a refitted node is too wide for the 64-byte form, that form is dropped as at build (has64 = 0, the
 *                               node format is decided again at the next render); a tree built without it does not gain one.
 *                               Unlike a rebuild it keeps the depth history of the beauty launches, the node-format verdict (while the
 *                               64-byte form survives), the ray, point, box, oriented box, frustum, triangle, sweep and segment queries' stack overflow areas (the tree's depth cannot change), the
 *                               AOVs, the denoiser's, temporal and adaptive state, and allocates nothing after the first refit on a
 *                               tree.  A tree whose root is a leaf refits its records only; a scene without triangles: MOPTIX_OK,
 *                               nothing done.  MOPTIX_ERR_STATE before moptix_build_accel.
 *                               moptix_denoise_temporal follows the moved triangles with the option "temporal_face_motion" = 1
 *                               (step 2 of its contract); by default a moved triangle is treated as static there.
 *   moptix_get_refit_info       of the last refit on this tree (zeros before the first):
 *     refitMs       device time of the refit's kernels (HIP events)
 *     sahCost       the sum over every child slot in use of every node of surface area(child box) x (1 for a node child, the triangle
 *                   count for a leaf child), divided by the surface area of the union of the root's child boxes, in binary64; 0 for a
 *                   tree without nodes
 *     sahCostBuilt  the same for the tree as built (taken at the first refit, before anything is overwritten)
 *     has64         1 while the tree has its 64-byte form
 *   sahCost / sahCostBuilt is a SIGNAL of how far the refitted boxes have grown beyond what a rebuild would choose; the library attaches
 *   no threshold to it. */
typedef struct { float refitMs; double sahCost, sahCostBuilt; uint32_t has64; } moptix_refit_info;
int moptix_update_faces(moptix_context ctx, int32_t firstFace, int32_t nFaces, const float* pos9, const float* nrm9);
int moptix_update_faces_device(moptix_context ctx, int32_t firstFace, int32_t nFaces, const float* dPos9, const float* dNrm9);
int moptix_refit_accel(moptix_context ctx);
int moptix_get_refit_info(moptix_context ctx, moptix_refit_info* out);

/* ---- measurement ----------------------------------------------------------- */
/* device time (HIP events on the launch stream) of the trace kernel -- the dominant kernel --
 * and the number of its launches since the last reset */
int moptix_kernel_time(moptix_context ctx, double* totalMs, uint64_t* nLaunches, int reset);
/* device time of the ordered sample reductions that followed those launches */
int moptix_reduce_time(moptix_context ctx, double* totalMs);

/* debug/validation: copy the built BVH to host (nodes: nNodes*128 B four-child nodes, tris: nTriangles*48 B,
 * triPrimIds: nTriangles int32 = original face index of each record). Any pointer may be NULL. */
int moptix_debug_read_accel(moptix_context ctx, void* nodes, void* tris, int32_t* triPrimIds);
/* the same nodes in the 64-byte form the trace kernels fetch (nNodes*64 B: corner, grid steps, 24 plane bytes, the four
 * child references -- csrc/pt_types.h Node64); node i of this array stands for node i of moptix_debug_read_accel's. */
int moptix_debug_read_nodes64(moptix_context ctx, void* nodes64);
/* A test aid, not an interface to build on: the addresses of buffers a call is documented to keep, so that a test can see that it
 * neither freed nor reallocated them (0 = not allocated).  out[0]: the ray queries' stack overflow area (device); out[1..6]: the refit
 * plan's device buffers (level order, per-triangle boxes, scene box, cost partials, cost, 64-byte verdict); out[7]: its pinned
 * read-back record (host).  Touches no device and no stream. */
int moptix_debug_buffer_addresses(moptix_context ctx, uint64_t out[8]);
/* nearest-hit query for n rays (BVH-vs-brute-force tests): rays = n x {ox,oy,oz,dx,dy,dz,tmin,tmax};
 * outT[n], outPrim[n] (prim id: spheres, quads, triangles; -1 = miss). */
int moptix_debug_trace(moptix_context ctx, const float* rays, int32_t n, float* outT, int32_t* outPrim);

#ifdef __cplusplus
}
#endif
#endif /* MOPTIX_H */
