// pt_counters.h -- the counter block of the counting build (LaunchArgs::counters), one name per word.
// Written by the trace kernels (the flush blocks at the end of pt_megakernel, pt_queuekernel, pt_packetkernel, pt_drainkernel and
// a few in-loop updates), cleared by do_render and decoded by read_stats (api_render.hip).  All words are unsigned 64-bit.
#pragma once
#include "pt_types.h"

namespace pt {

// the thirteen words of moptix_stats, in its order; the first kCntPerLane of them are summed over the lanes of a wave (LaneCounters)
constexpr int kCntSamples = 0, kCntPrimaryRays = 1, kCntBounceRays = 2, kCntShadowRays = 3, kCntNodeFetches = 4, kCntTriTests = 5,
              kCntClosestHits = 6, kCntLightLoads = 7, kCntAnalyticTests = 8, kCntPerLane = 9,
              kCntTraversalSteps = 9, kCntActiveLaneSteps = 10, kCntShadeBatches = 11, kCntShadeBatchLanes = 12;
// scheduler of the queue kernels: slots waiting in the wave's leaf ring / node ring at the start of a node run (sums), idle spins
constexpr int kCntLeafBacklog = 13, kCntIdleSpins = 14, kCntRingBacklog = 15;
// phase clocks (s_memtime ticks summed over the waves) and what they are divided by
constexpr int kCntTBatch = 16, kCntTSwap = 17, kCntTNode = 18, kCntTLeaf = 19, kCntTFinish = 20, kCntTWave = 21,
              kCntLeafPasses = 22, kCntLeafLanes = 23,
              kCntTLocal = 24, kCntTLock = 25, kCntTTxn = 26, kCntTIdle = 27, kCntTBatchLoad = 28, kCntTBatchRun = 29, kCntTBatchStore = 30,
              kCntTransactions = 31, kCntIterations = 32, kCntIterResult = 33, kCntIterLights = 34, kCntIterNewItem = 35;
// timeline of the launch (100 MHz s_memrealtime stamps): first wave in (min), first time the items ran out (min), last wave out (max).
// The two minima are adjacent: do_render presets them to all ones with one memset.
constexpr int kCntFirstWaveIn = 36, kCntItemsRanOut = 37, kCntLastWaveOut = 38;
constexpr int kCntNodeRuns = 39;
// samples finishing per millisecond after the first wave started, kCntTailBuckets buckets each: count, deepest path, sum of depths
constexpr int kCntTailBuckets = 256;
constexpr int kCntTailCount = 40, kCntTailMaxDepth = kCntTailCount + kCntTailBuckets, kCntTailDepthSum = kCntTailMaxDepth + kCntTailBuckets;
// slot-record rows (16 B) moved by the packet kernel: shading visit loads / stores, leaf pass loads / stores
constexpr int kCntSlotRows = kCntTailDepthSum + kCntTailBuckets;
// hand-over packet kernel -> drain kernel: paths handed over, paths taken, samples the drain kernel / the packet kernel finished
constexpr int kCntHandedOver = kCntSlotRows + 4, kCntDrainTaken = kCntHandedOver + 1, kCntDrainFinished = kCntHandedOver + 2, kCntPacketFinished = kCntHandedOver + 3;
// lane census of the divergent regions (pt_path.h census<>): lanes that entered, then waves that entered, kCensusRegions words each
constexpr int kCntCensusLanes = kCntHandedOver + 4, kCntCensusWaves = kCntCensusLanes + kCensusRegions;
constexpr int kCntTotal = kCntCensusWaves + kCensusRegions;

static_assert(kCntItemsRanOut == kCntFirstWaveIn + 1, "the two minima are preset by one memset");

}  // namespace pt
