// api_render.hip -- the beauty launches: which node format, which trace kernel and how large (the launch plan), the buffers the plan asks for,
// the launch loop, the counting build's report.  moptix_launch / render / render_async / render_counted / sync of include/moptix.h.
#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "api_context.h"
#include "pt_lanestack.h"

using namespace pt;
using namespace pt::api;

namespace {

// Which node record the packet kernel fetches for this scene.  The 64-byte form saves three of seven look-ups per node step but
// its boxes are a grid step larger.  Curved meshes hardly notice (coffee: +2 % node steps, +2 % triangle tests, frame -2.7 %);
// a ray that leaves a large axis-aligned face does -- the face's exact box is thinner than tmin and culls itself, its quantised
// box is a grid step of the PARENT thick and the ray starts inside it: the dining-room stand-in, whose walls are two triangles
// each, tests 17 % more triangles (it lost 6 % in round 3 and is level since round 4).  Static measures of the tree (surface-area inflation: 0.3 % for the dining
// room, 0.7 % for coffee) and synthetic rays miss this, so the scene is asked with its own paths: one sample per pixel of a
// 128-pixel-wide grid over the camera's view, cut at depth 6, walked under both forms; the counts are priced with the per-step
// costs fitted to coffee, the coffee pot, the glass knot and the dining room (a triangle test = 1.3 node steps of the
// 128-byte form; a 64-byte step = 0.93 of one since round 5, 0.78 in round 4).  Decided at the first render after a build or a change of frame size; a
// later change of camera keeps the verdict (moptix_set_params).
constexpr int kProbeWidth = 128;
int choose_node_format(moptix_context c) {
  c->formatDecided = true;
  c->nodeFormatUsed = 128;
  for (auto& v : c->probeCounts) v = 0;
  if (c->bvh.nNodes <= 0 || !c->bvh.nodes64) return MOPTIX_OK;      // no tree, or one without a 64-byte form (lbvh.h)
  if (c->opt.nodeFormat != 0) { c->nodeFormatUsed = c->opt.nodeFormat; return MOPTIX_OK; }
  SceneView v; fill_view(c, v);
  v.nodes64 = c->bvh.nodes64;
  const int w = std::min(kProbeWidth, v.width), h = std::max(1, (int)((long long)v.height * w / std::max(1, v.width)));
  v.width = w; v.height = h;
  const size_t threads = ((size_t)w * h + 255) / 256 * 256;
  unsigned long long* dOut = nullptr; int* dOvf = nullptr;
  hipError_t e = hipMalloc((void**)&dOut, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemsetAsync(dOut, 0, 4 * sizeof(unsigned long long), c->stream);
  const size_t ovf = lane_stack_overflow_entries(threads, c->bvh.stackBound, megakernel_lds_stack_entries());
  if (e == hipSuccess && ovf > 0) e = hipMalloc((void**)&dOvf, sizeof(int) * ovf);
  if (e == hipSuccess) e = launch_probe_paths(c->stream, v, 0, false, dOut, dOvf);
  if (e == hipSuccess) e = launch_probe_paths(c->stream, v, 0, true, dOut + 2, dOvf);
  if (e == hipSuccess) e = hipMemcpyAsync(c->probeCounts, dOut, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (dOut) (void)hipFree(dOut);
  if (dOvf) (void)hipFree(dOvf);
  if (e != hipSuccess) return hipFail(c, e, "node format probe");
  // Round 4 re-fit (profiles/r04_node_format.txt): the 64-byte step lost 45 instructions (sign-selected plane words) and the leaf pass
  // its dependent fetches, so a triangle test weighs 1.3 node steps instead of 3.5 and a 64-byte step 0.78 of a 128-byte one.
  const double cost128 = (double)c->probeCounts[0] + 1.3 * (double)c->probeCounts[1];
  // Round 5 re-fit (profiles/r05_node_format.txt): the 128-byte step is fetched by the ray's signs now (pt_path.h: no min / max per plane
  // pair), which makes it the cheaper step in instructions (100 against 130) and leaves the 64-byte one its four gathers against seven:
  // a 64-byte step = 0.93 of a 128-byte one.  Coffee, coffee + pot and the glass knot keep the 64-byte nodes (2-3 % faster), the dining
  // room -- whose quantised wall boxes cost it 17 % more triangle tests -- goes back to the 128-byte ones (38.7 against 40.6 ms).
  const double cost64 = 0.93 * (double)c->probeCounts[2] + 1.3 * (double)c->probeCounts[3];
  c->nodeFormatUsed = cost64 < cost128 ? 64 : 128;
  if (getenv("MOPTIX_DEBUG"))
    fprintf(stderr, "[moptix] node format probe (%dx%d paths): 128-byte nodes %llu steps %llu triangle tests, 64-byte %llu / %llu -> %d\n", w, h,
            c->probeCounts[0], c->probeCounts[1], c->probeCounts[2], c->probeCounts[3], c->nodeFormatUsed);
  return MOPTIX_OK;
}

// The MOPTIX_DEBUG report of a counted launch (tools/install_profiles.sh and tools/gpu_census.py read these lines).
void report_counters(const unsigned long long* h) {
  fprintf(stderr, "[moptix] batches %llu lanes %llu full %llu allidle %llu waitingSum %llu\n", h[kCntShadeBatches], h[kCntShadeBatchLanes], h[kCntLeafBacklog], h[kCntIdleSpins], h[kCntRingBacklog]);
  const double tt = (double)h[kCntTWave];
  fprintf(stderr, "[moptix] wave time: batch %.1f%% refill %.1f%% node %.1f%% leaf %.1f%% finish %.1f%% (steps %llu, cycles/wave %.3g)\n",
          100 * h[kCntTBatch] / tt, 100 * h[kCntTSwap] / tt, 100 * h[kCntTNode] / tt, 100 * h[kCntTLeaf] / tt, 100 * h[kCntTFinish] / tt, h[kCntTraversalSteps], tt);
  fprintf(stderr, "[moptix] idle spins %llu\n", h[kCntIdleSpins]);
  // absolute pass clocks (s_memtime ticks summed over the waves) with the launch's span in the same ticks per wave: for a launch that
  // is one path walking (tools/gpu_lone_path.py) the passes are serial, so span - (batch + node + leaf) is what the scheduler costs
  if (h[kCntLastWaveOut] && h[kCntFirstWaveIn] != ~0ull && h[kCntLastWaveOut] > h[kCntFirstWaveIn])
    fprintf(stderr, "[moptix] pass ticks: batch %llu (load %llu run %llu store %llu) node %llu leaf %llu txn %llu lock %llu local %llu idle %llu | waves' time %llu over a span of %.1f us | "
                    "batches %llu node runs %llu leaf passes %llu iterations %llu transactions %llu\n", h[kCntTBatch], h[kCntTBatchLoad], h[kCntTBatchRun], h[kCntTBatchStore], h[kCntTNode], h[kCntTLeaf], h[kCntTTxn], h[kCntTLock], h[kCntTLocal], h[kCntTIdle], h[kCntTWave],
            (double)(h[kCntLastWaveOut] - h[kCntFirstWaveIn]) * 1e-2, h[kCntShadeBatches], h[kCntNodeRuns], h[kCntLeafPasses], h[kCntIterations], h[kCntTransactions]);
  if (h[kCntIterations]) fprintf(stderr, "[moptix] swap detail: local %.1f%% lock-wait %.1f%% txn %.1f%% idle %.1f%% | batch detail: load %.1f%% run %.1f%% store %.1f%% | "
                     "iterations %llu transactions %llu (cycles/iter %.0f)\n", 100 * h[kCntTLocal] / tt, 100 * h[kCntTLock] / tt, 100 * h[kCntTTxn] / tt, 100 * h[kCntTIdle] / tt,
                     100 * h[kCntTBatchLoad] / tt, 100 * h[kCntTBatchRun] / tt, 100 * h[kCntTBatchStore] / tt, h[kCntIterations], h[kCntTransactions], tt / (double)h[kCntIterations]);
  if (h[kCntLastWaveOut]) fprintf(stderr, "[moptix] timeline (100 MHz clock): items ran out %.2f ms after the first wave started, last wave left %.2f ms after that\n",
                     (double)(h[kCntItemsRanOut] - h[kCntFirstWaveIn]) * 1e-5, (double)(h[kCntLastWaveOut] - h[kCntItemsRanOut]) * 1e-5);
  if (h[kCntLastWaveOut]) {
    int lastB = 0; for (int b = 0; b < kCntTailBuckets; b++) if (h[kCntTailCount + b]) lastB = b;
    const int ranOut = (int)((double)(h[kCntItemsRanOut] - h[kCntFirstWaveIn]) * 1e-5);
    fprintf(stderr, "[moptix] samples finishing per ms from the moment the items ran out (count, mean depth, max depth):");
    for (int b = ranOut > 2 ? ranOut - 2 : 0; b <= lastB; b++)
      fprintf(stderr, " [%d: %llu %.1f %llu]", b, h[kCntTailCount + b], h[kCntTailCount + b] ? (double)h[kCntTailDepthSum + b] / (double)h[kCntTailCount + b] : 0.0, h[kCntTailMaxDepth + b]);
    fprintf(stderr, "\n");
  }
  if (h[kCntNodeRuns]) fprintf(stderr, "[moptix] node runs %llu: node-ready slots waiting in the wave's ring %.1f, leaf ring %.1f (averages at the start of a run)\n",
                     h[kCntNodeRuns], (double)h[kCntRingBacklog] / (double)h[kCntNodeRuns], (double)h[kCntLeafBacklog] / (double)h[kCntNodeRuns]);
  if (h[kCntIterations]) fprintf(stderr, "[moptix] batch iterations executing on_result %llu, on_lights %llu, new item %llu (batches %llu)\n", h[kCntIterResult], h[kCntIterLights], h[kCntIterNewItem], h[kCntShadeBatches]);
  if ((h[kCntSlotRows] | h[kCntSlotRows + 1])) {
    const double rays = (double)(h[kCntPrimaryRays] + h[kCntBounceRays] + h[kCntShadowRays]);
    fprintf(stderr, "[moptix] slot-record rows (16 B each) per ray: shading visit loads %.2f stores %.2f | leaf pass loads %.2f stores %.2f | total %.1f B per ray in %.2f shading visits and %.2f leaf visits per ray\n",
            h[kCntSlotRows] / rays, h[kCntSlotRows + 1] / rays, h[kCntSlotRows + 2] / rays, h[kCntSlotRows + 3] / rays, 16.0 * (double)(h[kCntSlotRows] + h[kCntSlotRows + 1] + h[kCntSlotRows + 2] + h[kCntSlotRows + 3]) / rays, (double)h[kCntShadeBatchLanes] / rays, (double)h[kCntLeafLanes] / rays);
  }
  if ((h[kCntHandedOver] | h[kCntDrainTaken])) fprintf(stderr, "[moptix] hand-over: %llu paths handed over by the packet kernel, %llu taken by the drain kernel; samples finished: %llu by the packet kernel + %llu by the drain kernel (of %llu)\n", h[kCntHandedOver], h[kCntDrainTaken], h[kCntPacketFinished], h[kCntDrainFinished], h[kCntSamples]);
  if (h[kCntLeafPasses]) fprintf(stderr, "[moptix] node steps %llu (%.1f lanes avg), leaf passes %llu (%.1f lanes avg)\n", h[kCntTraversalSteps] - h[kCntLeafPasses],
          (double)(h[kCntActiveLaneSteps] - h[kCntLeafLanes]) / (double)(h[kCntTraversalSteps] - h[kCntLeafPasses]), h[kCntLeafPasses], (double)h[kCntLeafLanes] / (double)h[kCntLeafPasses]);
  if (h[kCntCensusWaves]) {      // lane census of the divergent regions (pt_path.h census<>)
    static const char* names[kCensusRegions] = { "result visit (on_result_packet)", "  miss", "  closest hit (hit_attributes + material)", "    light material",
      "    depth cap", "    lambertian", "    metal", "    glass", "    disney GLASS", "    disney (on_lights_packet)", "      light 0 faces: pdf + eval", "      light 1 faces: pdf + eval",
      "      light 2 faces: pdf + eval", "      bounce: pdf + eval", "new work item (begin_sample)", "leaf pass: triangle 0 tested", "leaf pass: triangle 1 tested",
      "leaf pass: triangle 2 tested", "leaf pass: triangle 3 tested", "  triangle hit accepted by tri_test", "  shadow result folded", "      light draw (per light)", "      bounce: disney_sample", "node step: branched tail (stack nearly full)" };
    fprintf(stderr, "[moptix] lane census: region | waves that entered | lanes that entered | lanes per wave (of 64)\n");
    for (int i = 0; i < kCensusRegions; i++)
      if (h[kCntCensusWaves + i]) fprintf(stderr, "[moptix]   %-46s %12llu %14llu %6.1f\n", names[i], h[kCntCensusWaves + i], h[kCntCensusLanes + i], (double)h[kCntCensusLanes + i] / (double)h[kCntCensusWaves + i]);
  }
}

int read_stats(moptix_context c, moptix_stats* stats) {
  unsigned long long h[kCntTotal] = {};
  HIPCHK(c, hipMemcpy(h, c->dCounters.p, sizeof(h), hipMemcpyDeviceToHost), "read counters");      // do_render allocated and cleared the whole block
  stats->samples = h[kCntSamples]; stats->primaryRays = h[kCntPrimaryRays]; stats->bounceRays = h[kCntBounceRays]; stats->shadowRays = h[kCntShadowRays];
  stats->nodeFetches = h[kCntNodeFetches]; stats->triTests = h[kCntTriTests]; stats->closestHits = h[kCntClosestHits]; stats->lightLoads = h[kCntLightLoads];
  stats->analyticTests = h[kCntAnalyticTests]; stats->traversalSteps = h[kCntTraversalSteps]; stats->activeLaneSteps = h[kCntActiveLaneSteps];
  stats->shadeBatches = h[kCntShadeBatches]; stats->shadeBatchLanes = h[kCntShadeBatchLanes];
  // timeline of a counted launch (100 MHz s_memrealtime stamps of the queue kernels): options "counted_span_us" / "counted_tail_us"
  c->countedSpanUs = -1; c->countedTailUs = -1;
  if (h[kCntLastWaveOut] && h[kCntFirstWaveIn] != ~0ull) { c->countedSpanUs = (int)((h[kCntLastWaveOut] - h[kCntFirstWaveIn]) / 100); c->countedTailUs = (h[kCntItemsRanOut] != ~0ull && h[kCntLastWaveOut] > h[kCntItemsRanOut]) ? (int)((h[kCntLastWaveOut] - h[kCntItemsRanOut]) / 100) : 0; }
  if (getenv("MOPTIX_DEBUG")) report_counters(h);
  return MOPTIX_OK;
}

// ---- the launch plan: what one batch of launches will run, decided from the context, the batch size and whether it counts ------------
// plan_launch touches neither the device nor the context's buffers; prepare_launch allocates what the plan (api_context.h LaunchPlan) asks
// for and launch_pass launches it.  byPixelSlots: the plan of an adaptive pass (api_adaptive.hip).
int plan_launch(moptix_context c, const SceneView& scene, int32_t nSeeds, bool counted, bool byPixelSlots, LaunchPlan& p) {
  memset(&p, 0, sizeof(p));
  const int tilesX = ((int)c->params.width + 7) / 8, tilesY = ((int)c->params.height + 7) / 8;
  const long long nTiles = (long long)tilesX * tilesY;
  const long long localTiles = (nTiles + c->nRanks - 1) / c->nRanks;     // one tile of every group of nRanks (megakernel.h item_to_pixel)
  if (localTiles * 64 > 0x7fffffffLL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  p.nItems = (int)(localTiles * 64); p.tilesX = tilesX;
  if (p.nItems == 0) return MOPTIX_OK;
  const long long budget = (long long)c->opt.sampleBufMB << 20;
  p.perPass = budget / ((long long)p.nItems * 12);
  p.nBlocks = c->numCUs * c->opt.blocksPerCU;
  // the work counter is a 32-bit int that every path slot bumps once more after the items ran out
  const long long counterSlack = (long long)c->numCUs * std::max(4, c->opt.blocksPerCU) * 1024 + 65536;      // the lean queue kernel runs four workgroups per CU
  if ((long long)p.nItems + counterSlack > 0x7fffffffLL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  p.perPass = std::min(p.perPass, (0x7fffffffLL - counterSlack) / p.nItems);
  p.perPass = std::max(1LL, std::min(p.perPass, (long long)nSeeds));

  const bool hasTris = scene.rootRef != kEmptyRef;
  // Scenes without triangles ("NoAccel"): the per-lane kernel, or ("analytic_queue" = 1) the queue kernel, where every ray
  // is finished by the brute-force lists at set-up, inside a full 64-lane batch, and the slots cycle through the batches.
  // With the lists read by scalar loads, four spheres per trip (pt_path.h trav_begin): random_spheres (497 + 33 primitives)
  // 60.6 ms per-lane, 47.8 ms queue (round 1: 92.3); cornell_quads (16 quads) 15.0 / 17.3 ms.  -1 = queue from 64 primitives on.
  const bool analyticQueue = c->opt.analyticQueue >= 0 ? c->opt.analyticQueue != 0 : (c->spheres.size() + c->quads.size() >= 64);
  // variant 4 (packetkernel.hip, one shading visit per bounce): triangle scenes with at most three lights and no Disney
  // material on an analytic primitive; anything else runs on variant 3.
  // "auto_packet" (default on): while "kernel_variant" has not been set, variant 4 is what such a scene runs on from 1e6
  // samples and 16 launches on.  Its paths have the shorter critical path (one rank's share of an 8-way split of the
  // benchmark frame: 66.7 against 78.4 ms) and, since the scene tables are read as constants (pt_types.h load_uniform),
  // its visits are the cheaper ones as well: whole frame 442 against 452 ms, dining room at 64 spp 162 against 193 ms.
  const bool packetOk = hasTris && scene.nLights <= 3 && !scene.anyDisneyAnalytic;
  const double nSamples = (double)p.nItems * (double)nSeeds;
  // (until round 4 mostly-glass scenes stayed on variant 3: no shadow rays to pack, and variant 4's wider records cost 10 % there; with
  // this round's leaf pass and routing the two are level on the glass knot -- 56.2 against 57.0 ms -- so the packet kernel serves both)
  const bool autoPacket = nSamples >= 1.0e6 && nSeeds >= 16;
  const bool variantExplicit = c->opt.kernelVariant >= 0;      // "kernel_variant" was set by the caller: no automatic choice
  const int variant = variantExplicit ? c->opt.kernelVariant : 3;
  const bool usePacket = packetOk && (variant == 4 || (!variantExplicit && c->opt.autoPacket != 0 && autoPacket));
  // (an adaptive pass hands its pixels out through handout_to_item, which the per-lane kernel does not go through: a queue kernel stands in)
  const bool useQueue = !usePacket && (byPixelSlots || ((variant >= 3) && (hasTris || analyticQueue)));
  p.kernel = usePacket ? &kPacketKernel : !useQueue ? nullptr : hasTris ? &kQueueKernel : &kLeanQueueKernel;      // scenes without triangles: queuekernel_lean.hip
  p.variant = usePacket ? 4 : useQueue ? 3 : 0;
  // the packet kernel has a build without the programs this scene's tables cannot reach (packetkernel.hip; option "specialize" 0: never)
  // (its hit records, pt_types.h TriFace, are addressed by a 32-bit byte offset from the TriShade array they follow: where the two arrays together reach
  // 4 GB -- above 38 million triangles -- the scene runs the general build)
  const bool faceTableOk = (unsigned long long)tri_face_offset(0) + (unsigned long long)scene.nTris * (sizeof(TriShade) + sizeof(TriFace)) + 64ull < (1ull << 32);
  const int features = (usePacket && c->opt.specialize != 0 && faceTableOk) ? scene_features(c) : FEAT_ALL;
  // no tree to walk (queuekernel_lean.hip): a fourth workgroup per CU instead of path slots and stack entries
  if (p.kernel == &kLeanQueueKernel && c->opt.blocksPerCU == 3) p.nBlocks = c->numCUs * 4;
  // Slots without a path are what deep paths borrow for their shadow rays (packetkernel.hip, "aux_depth"); once the work
  // items run out there are plenty, before that only the ones kept free here.  A launch under 1e8 samples (an 8-way share
  // of the benchmark frame) is short enough for its tail to matter more than the throughput of 64 more paths per pool:
  // 66.7 ms with 448 of 512 slots in use against 70.1 ms with all of them; a 4-way share: 130.3 against 125.0 ms.
  // A scene that is mostly glass has hardly any shadow rays to borrow slots for: all slots carry paths there (glass knot at 16 spp: 53.9 against 55.9 ms).
  p.slotsInUse = c->opt.slotsInUse >= 0 ? c->opt.slotsInUse : (usePacket && c->opt.auxDepth > 0 && nSamples < 1.0e8 && c->glassFaceShare <= 0.5 ? packetkernel_slots() * 7 / 8 : 0);
  // A launch of 1e8 samples or more whose slots are not the caller's choice keeps none free (above), so nothing can be borrowed before the work items
  // run out, and the paths that are left then go to the drain kernel: such a launch runs without borrowed slots.  (Measured on the benchmark frame,
  // profiles/r21_slim_isa.txt: "aux_depth" 0 against 16 in the same kernel, warm frame 301.03 against 301.73 ms, a context's first frame 306.98
  // against 307.62 ms -- not slower in either, so the rule does not ask for a depth history.)
  p.auxDepth = usePacket ? c->opt.auxDepth : 0;
  if (usePacket && c->opt.slotsInUse < 0 && nSamples >= 1.0e8) p.auxDepth = 0;
  if (usePacket) {
    // variant 4: the packet kernel's workgroups hand their last paths to the drain kernel (drainkernel.hip; "drain_below" = 0 keeps them in the packet kernel)
    // (not under "shadow_rule" 0 in a scene with glass: there a shadow ray's attenuation is a PRODUCT over the glass surfaces it crosses, taken in
    // traversal order, and the drain kernel's order is not the packet kernel's)
    bool glassMaterial = false;
    for (const DevMaterial& m : c->mats) if (m.kind == MAT_DISNEY && m.brdfType == BRDF_GLASS) glassMaterial = true;
    p.drainBelow = (glassMaterial && !scene.shadowNearest) ? 0 : c->opt.drainBelow;
    // The slim build of the lean kernel (packetkernel.hip: AUX = false, GLASS = NEAR) holds no borrowed-slot machinery and, where shadow rays do not keep
    // their nearest candidate, no Disney GLASS code: a lean launch runs it when it borrows no slot and the material TABLE has no Disney GLASS entry
    // (glass under "shadow_rule" 0 has shadowNearest false and tinted attenuations: the NEAR = false slim kernel is not for it).  Same image bits
    // in every build.
    const bool slimEligible = p.auxDepth == 0 && (scene.shadowNearest || !glassMaterial);
    p.build = packet_build(counted, c->opt.fastShading != 0, features, slimEligible);
  }
  if (p.kernel) {
    p.ovfDepth = hasTris ? std::max(0, c->bvh.stackBound - p.kernel->lds_stack_entries() + 1) : 0;
    p.overflowInts = p.ovfDepth > 0 ? p.kernel->overflow_ints(p.nBlocks, p.ovfDepth) : 0;
    p.poolBytes = p.kernel->cold_bytes(p.nBlocks);
  } else {      // per thread, not per slot; LaunchArgs::ovfDepth stays 0
    p.overflowInts = lane_stack_overflow_entries((size_t)p.nBlocks * 256, c->bvh.stackBound, megakernel_lds_stack_entries());
  }
  // the hand-out constants (megakernel.h HandoutConsts), then [0] work counter, [1] watchdog flag, then (variant 4) the drain list
  // (megakernel.h kDrain*): counters, capacity, threshold, entries; LaunchArgs::workCounter points at [0]
  p.workInts = kHandoutWords + 2 + drain_list_ints(p.nBlocks, p.drainBelow);
  p.tileMajor = byPixelSlots ? 3 : p.kernel ? c->opt.tileMajor : 0;
  p.unitShift = p.tileMajor == 3 ? 0 : 6;
  p.historyUnits = (localTiles * 64) >> p.unitShift;
  return MOPTIX_OK;
}

// MOPTIX_DEBUG: how the deepest-path history is distributed over the tiles
int report_tile_history(moptix_context c) {
  std::vector<unsigned int> cost((size_t)c->tiles.units);
  HIPCHK(c, hipMemcpy(cost.data(), c->tiles.keys.p, sizeof(unsigned int) * cost.size(), hipMemcpyDeviceToHost), "read tile cost");
  size_t hist[6] = { 0, 0, 0, 0, 0, 0 };                        // 0, 8..15, 16..63, 64..255, 256+, first half of the tiles holding 256+
  for (size_t i = 0; i < cost.size(); i++) {
    const unsigned int v = cost[i];
    hist[v == 0 ? 0 : v < 16 ? 1 : v < 64 ? 2 : v < 256 ? 3 : 4]++;
    if (v >= 256 && i < cost.size() / 2) hist[5]++;
  }
  fprintf(stderr, "[moptix] depth history (%zu units): none %zu, depth 8-15 %zu, 16-63 %zu, 64-255 %zu, capped %zu (of which %zu in the first half)\n",
          cost.size(), hist[0], hist[1], hist[2], hist[3], hist[4], hist[5]);
  return MOPTIX_OK;
}

#ifdef PT_EVLOG      // experiment build only (packetkernel.hip PT_EV): the event log stands in for the counters of an UNCOUNTED launch
constexpr size_t kEvLogWords = 65536;
int evlog_begin(moptix_context c, DevBuf<unsigned long long>& evLog, LaunchArgs& a) {
  HIPCHK(c, evLog.ensure(kEvLogWords + 8), "alloc event log");      // always there: the kernel logs whenever it meets a path deeper than 100 bounces
  HIPCHK(c, hipMemsetAsync(evLog.p, 0, sizeof(unsigned long long) * (kEvLogWords + 8), c->stream), "zero event log");
  a.evLog = evLog.p;
  return MOPTIX_OK;
}
int evlog_write(moptix_context c, const DevBuf<unsigned long long>& evLog) {      // tools/evlog_timeline.py reads the file
  std::vector<unsigned long long> h(kEvLogWords);
  HIPCHK(c, hipMemcpy(h.data(), evLog.p, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost), "read event log");
  FILE* f = fopen(getenv("MOPTIX_EVLOG"), "wb");
  if (f) { fwrite(h.data(), sizeof(unsigned long long), (size_t)std::min<unsigned long long>(h[0], 65000ull) + 1, f); fclose(f); }
  return MOPTIX_OK;
}
#endif

}  // namespace

namespace pt { namespace api {

// The context's pinned staging, at least `ints` long and free to be written: whatever was copied from it last has left it.  That is the
// only wait: an asynchronous render behind a busy stream does not wait for the stream.
static int launch_staging(moptix_context c, size_t ints) {
  if (!c->launchStaged) HIPCHK(c, hipEventCreateWithFlags(&c->launchStaged, hipEventDisableTiming), "create event");
  else HIPCHK(c, hipEventSynchronize(c->launchStaged), "wait for the previous batch's uploads");
  if (c->launchStagingInts < ints) {
    if (c->launchStaging) (void)hipHostFree(c->launchStaging);
    c->launchStaging = nullptr; c->launchStagingInts = 0;
    HIPCHK(c, hipHostMalloc((void**)&c->launchStaging, sizeof(int) * ints, hipHostMallocDefault), "alloc launch staging");
    c->launchStagingInts = ints;
  }
  return MOPTIX_OK;
}

int prepare_launch(moptix_context c, int32_t nSeeds, bool counted, bool byPixelSlots, RenderLaunch& r) {
  int rc;
  if (!c->formatDecided && (rc = choose_node_format(c)) != MOPTIX_OK) return rc;
  LaunchArgs& a = r.a;
  LaunchPlan& p = r.p;
  memset(&a, 0, sizeof(a));
  fill_view(c, a.scene);
  if ((rc = plan_launch(c, a.scene, nSeeds, counted, byPixelSlots, p)) != MOPTIX_OK || p.nItems == 0) return rc;
  c->lastVariant = p.variant;
  r.counted = counted; r.fast = c->opt.fastShading != 0;
  c->lastFeatures = p.build == PacketBuild::General ? FEAT_ALL : 0;
  c->lastSlim = p.build == PacketBuild::Slim ? 1 : 0;

  // ---- what the plan asks for ----
  a.accum = accum_ptr(c);
  a.nItems = p.nItems; a.tilesX = p.tilesX; a.rank = c->rank; a.nRanks = c->nRanks;
  a.exitThreshold = c->opt.exitThreshold; a.leafThreshold = c->opt.leafThreshold;
  a.starveLanes = c->opt.starveLanes; a.swapLanes = c->opt.swapLanes;
  a.slotsInUse = p.slotsInUse; a.auxDepth = p.auxDepth; a.ovfDepth = p.ovfDepth;
  a.watchdogTicks = (unsigned long long)c->opt.watchdogMs * 100000ull;      // s_memrealtime counts at 100 MHz
  if (p.overflowInts > 0) {
    HIPCHK(c, c->dOverflow.ensure(p.overflowInts), "alloc stack overflow area");
    a.stackOverflow = c->dOverflow.p;
  }
  if (p.kernel) {
    HIPCHK(c, c->dPoolCold.ensure(p.poolBytes), "alloc path pool");
    a.poolCold = c->dPoolCold.p;
  }
  // the per-sample buffer is the one large allocation (up to "sample_buffer_mb", 16 GB by default; two pipelined contexts
  // hold one each): when the device cannot give it, run more and smaller passes instead of failing the render
  long long perPass = p.perPass;
  for (;;) {
    const hipError_t e = c->dSampleBuf.ensure((size_t)perPass * a.nItems * 3);
    if (e == hipSuccess) break;
    if (e != hipErrorOutOfMemory || perPass <= 1) return hipFail(c, e, "alloc per-sample buffer");
    (void)hipGetLastError();
    perPass = (perPass + 1) / 2;
  }
  r.perPass = perPass;
  a.sampleBuf = c->dSampleBuf.p;
  HIPCHK(c, c->dWork.ensure(p.workInts), "alloc work counter");
  {
    // the first pass takes min(perPass, nSeeds) seeds: its hand-out constants travel with the header (launch_pass writes them again for a pass of another size)
    struct { HandoutConsts hc; int hdr[2 + kDrainEntries]; } w = { handout_consts(p.tileMajor, a.nItems, (int)std::min<long long>(perPass, nSeeds), a.tilesX, a.nRanks),
                                                                   { 0, 0, 0, 0, 0, 0, p.nBlocks * p.drainBelow, p.drainBelow } };
    static_assert(sizeof(w) == sizeof(int) * (kHandoutWords + 2 + kDrainEntries), "the work header is packed");
    // through the pinned staging (the header, then room for the seeds): the copy is asynchronous and nothing here waits for the stream
    if ((rc = launch_staging(c, sizeof(w) / sizeof(int) + (size_t)nSeeds)) != MOPTIX_OK) return rc;
    memcpy(c->launchStaging, &w, sizeof(w));
    r.seedStaging = c->launchStaging + sizeof(w) / sizeof(int);
    HIPCHK(c, hipMemcpyAsync(c->dWork.p, c->launchStaging, sizeof(w), hipMemcpyHostToDevice, c->stream), "init work counter");
    HIPCHK(c, hipEventRecord(c->launchStaged, c->stream), "event");
    r.handoutDivisor = handout_divisor(p.tileMajor, a.nItems, (int)std::min<long long>(perPass, nSeeds)); r.handoutSeeds = (int)std::min<long long>(perPass, nSeeds);
  }
  a.workCounter = c->dWork.p + kHandoutWords;
  a.tileMajor = p.tileMajor; a.unitShift = p.unitShift;
  if (p.tileMajor) {
    HIPCHK(c, c->tiles.ensure(p.historyUnits, c->stream), "start depth history");      // new frame size / partition / granularity: afresh
    a.tileOrder = c->tiles.order.p; a.tileCost = c->tiles.keys.p;
  }
  if (counted) {
    HIPCHK(c, c->dCounters.ensure(kCntTotal), "alloc counters");
    HIPCHK(c, hipMemsetAsync(c->dCounters.p, 0, sizeof(unsigned long long) * kCntTotal, c->stream), "zero counters");
    HIPCHK(c, hipMemsetAsync(c->dCounters.p + kCntFirstWaveIn, 0xff, sizeof(unsigned long long) * 2, c->stream), "init min counters");      // and kCntItemsRanOut
    a.counters = c->dCounters.p;
  }
  return MOPTIX_OK;
}

// ---- OrderList (api_context.h).  rocprim's radix sort of (key, id) pairs, descending and stable (ties stay in id order), is instantiated
// here alone: tmp == nullptr sets only tmpBytes, the scratch the sort needs.
static hipError_t sort_pairs_desc(void* tmp, size_t& tmpBytes, OrderList& l, size_t n, hipStream_t stream) {
  return rocprim::radix_sort_pairs_desc(tmp, tmpBytes, l.keys.p, l.keysSorted.p, l.iota.p, l.order.p, n, 0, 32, stream);
}

hipError_t OrderList::ensure(long long n, hipStream_t stream) {
  if (units == n) return hipSuccess;
  units = -1;
  std::vector<int> ids((size_t)n);
  for (size_t i = 0; i < ids.size(); i++) ids[i] = (int)i;
  hipError_t e = keys.ensure((size_t)n);
  if (e == hipSuccess) e = keysSorted.ensure((size_t)n);
  if (e == hipSuccess) e = order.ensure((size_t)n);
  if (e == hipSuccess) e = iota.upload(ids, stream);
  if (e == hipSuccess) e = hipMemsetAsync(keys.p, 0, sizeof(unsigned int) * (size_t)n, stream);
  size_t tmpBytes = 0;
  if (e == hipSuccess) e = sort_pairs_desc(nullptr, tmpBytes, *this, (size_t)n, stream);
  if (e == hipSuccess) e = sortTmp.ensure(tmpBytes);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);      // ids dies here
  if (e == hipSuccess) units = n;
  return e;
}

hipError_t OrderList::sort(hipStream_t stream) {
  size_t tmpBytes = sortTmp.n;
  return sort_pairs_desc(sortTmp.p, tmpBytes, *this, (size_t)units, stream);
}

int launch_pass(moptix_context c, RenderLaunch& r, const int* dSeeds, int n, const PassOverride* over) {
  LaunchArgs& a = r.a;
  const LaunchPlan& p = r.p;
  a.seeds = dSeeds; a.nSeeds = n; a.nWork = over ? over->nWork : n * a.nItems;
  if (handout_divisor(a.tileMajor, a.nItems, n) != r.handoutDivisor || n != r.handoutSeeds) {      // a pass of another size than the last (a batch's remainder, an adaptive pass): its own constants
    const HandoutConsts hc = handout_consts(a.tileMajor, a.nItems, n, a.tilesX, a.nRanks);
    HIPCHK(c, hipMemcpyAsync(a.workCounter - kHandoutWords, &hc, sizeof(hc), hipMemcpyHostToDevice, c->stream), "write hand-out constants");
    HIPCHK(c, hipStreamSynchronize(c->stream), "sync");      // hc lives on this stack frame
    r.handoutDivisor = handout_divisor(a.tileMajor, a.nItems, n); r.handoutSeeds = n;
  }
  HIPCHK(c, hipMemsetAsync(a.workCounter, 0, (2 + kDrainCap) * sizeof(int), c->stream), "zero work counter");      // counters only: capacity and threshold stay
  if (over) a.tileOrder = over->order;
  else if (a.tileMajor && a.tileCost) HIPCHK(c, c->tiles.sort(c->stream), "sort tiles");      // deepest path seen so far first, ties in raster order
  HIPCHK(c, hipEventRecord(c->ev0, c->stream), "event");
  if (p.kernel) HIPCHK(c, p.kernel->launch(c->stream, a, p.nBlocks, r.counted, r.fast, p.build), p.kernel->launchWhat);
  else HIPCHK(c, launch_megakernel(c->stream, a, p.nBlocks, r.counted), "launch megakernel");
  if (p.drainBelow > 0) HIPCHK(c, launch_drainkernel(c->stream, a, c->numCUs, r.counted, r.fast), "launch drain kernel");
  // Since the drain kernel came, a packet launch WITHOUT it ("drain_below" 0) has been followed by the per-lane megakernel: it finds the work counter
  // used up and leaves at once.  Nothing needs that launch; it stays until a change of its own takes it out, so that the launches are what they were.
  else if (p.kernel == &kPacketKernel) HIPCHK(c, launch_megakernel(c->stream, a, p.nBlocks, r.counted), "launch megakernel");
  HIPCHK(c, hipEventRecord(c->ev1, c->stream), "event");
  if (over) HIPCHK(c, over->reduce(c->stream, a, over->user), "launch adaptive reduction");
  else HIPCHK(c, launch_reduce_samples(c->stream, a), "launch sample reduction");
  HIPCHK(c, hipEventRecord(c->ev2, c->stream), "event");
  c->asyncPending = true;
  return MOPTIX_OK;
}

}}  // namespace pt::api

namespace {

// One batch of launches = [trace kernel: every (pixel, sample) work item -> per-sample buffer]
// + [ordered reduction: accuBuffer[pixel] += samples in launch order].  Batches larger than the
// sample-buffer budget (or 2^31 work items) are cut into passes of whole launches.
int do_render(moptix_context c, const int32_t* seeds, int32_t nSeeds, bool counted, bool blocking, moptix_stats* stats) {
  int rc = check_ready(c);
  if (rc != MOPTIX_OK) return rc;
  if (nSeeds < 0 || (nSeeds > 0 && !seeds)) return fail(c, MOPTIX_ERR_INVALID, "bad seeds");
  if (c->ad.have) return fail(c, MOPTIX_ERR_STATE, "the accumulation buffer holds an adaptive render (per-pixel sample counts): moptix_adaptive_clear or moptix_accum_clear first");
  // An asynchronous render with no batch in flight is ordered by the stream alone and does not wait for it (include/moptix.h: "non-blocking
  // variant for stream overlap"); with one in flight that batch finishes and is timed first, as for every other call.
  if (blocking || c->asyncPending) rc = begin_call(c, true);
  else { HIPCHK(c, hipSetDevice(c->device), "hipSetDevice"); rc = ensure_accum(c); }
  if (rc != MOPTIX_OK) return rc;
  if (nSeeds == 0) return MOPTIX_OK;
  RenderLaunch r;
  if ((rc = prepare_launch(c, nSeeds, counted, false, r)) != MOPTIX_OK || r.p.nItems == 0) return rc;
#ifdef PT_EVLOG
  DevBuf<unsigned long long> evLog;
  if ((rc = evlog_begin(c, evLog, r.a)) != MOPTIX_OK) return rc;
#endif
  memcpy(r.seedStaging, seeds, sizeof(int) * (size_t)nSeeds);   // pinned, in the context: the copy below may still be in flight when an async render returns
  HIPCHK(c, c->dSeeds.ensure((size_t)nSeeds), "alloc seeds");
  HIPCHK(c, hipMemcpyAsync(c->dSeeds.p, r.seedStaging, sizeof(int) * (size_t)nSeeds, hipMemcpyHostToDevice, c->stream), "upload seeds");
  HIPCHK(c, hipEventRecord(c->launchStaged, c->stream), "event");
  c->accumPlain = true;

  // ---- the launches ----
  for (long long first = 0; first < nSeeds; first += r.perPass) {
    const int n = (int)std::min(r.perPass, (long long)nSeeds - first);
    if ((rc = launch_pass(c, r, c->dSeeds.p + first, n, nullptr)) != MOPTIX_OK) return rc;
    const bool last = first + r.perPass >= nSeeds;
    if (!last || blocking) { if ((rc = moptix_sync(c)) != MOPTIX_OK) return rc; }
  }
#ifdef PT_EVLOG
  if (blocking && !counted && getenv("MOPTIX_EVLOG") && (rc = evlog_write(c, evLog)) != MOPTIX_OK) return rc;
  evLog.release();
#endif
  if (blocking && r.a.tileCost && getenv("MOPTIX_DEBUG") && (rc = report_tile_history(c)) != MOPTIX_OK) return rc;
  if (blocking && counted && stats) return read_stats(c, stats);
  return MOPTIX_OK;
}

}  // namespace

extern "C" {

int moptix_launch(moptix_context c, int32_t randSeed) { return do_render(c, &randSeed, 1, false, true, nullptr); }
int moptix_render(moptix_context c, const int32_t* seeds, int32_t nSeeds) { return do_render(c, seeds, nSeeds, false, true, nullptr); }
int moptix_render_async(moptix_context c, const int32_t* seeds, int32_t nSeeds) { return do_render(c, seeds, nSeeds, false, false, nullptr); }
int moptix_render_counted(moptix_context c, const int32_t* seeds, int32_t nSeeds, moptix_stats* out) {
  if (out) memset(out, 0, sizeof(*out));
  return do_render(c, seeds, nSeeds, true, true, out);
}

int moptix_sync(moptix_context c) {
  if (!c) return MOPTIX_ERR_INVALID;
  HIPCHK(c, hipStreamSynchronize(c->stream), "stream synchronize");
  if (c->asyncPending) {
    float ms = 0.f, ms2 = 0.f;
    if (hipEventElapsedTime(&ms, c->ev0, c->ev1) == hipSuccess) { c->kernelMs += ms; c->nLaunches++; }
    if (hipEventElapsedTime(&ms2, c->ev1, c->ev2) == hipSuccess) c->reduceMs += ms2;
    c->asyncPending = false;
    int flags[2] = { 0, 0 };
    if (c->dWork.p) HIPCHK(c, hipMemcpy(flags, c->dWork.p + kHandoutWords, sizeof(flags), hipMemcpyDeviceToHost), "read watchdog flag");
    if (flags[1] != 0) return fail(c, MOPTIX_ERR_HIP, "render kernel hit its watchdog (option watchdog_ms); this pass was not added to accuBuffer");
  }
  return MOPTIX_OK;
}

}  // extern "C"
