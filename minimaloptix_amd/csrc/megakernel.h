// megakernel.h -- launch interface of megakernel.hip
#pragma once
#include <hip/hip_runtime.h>
#include "pt_counters.h"
#include "pt_types.h"

namespace pt {

struct LaunchArgs {
  SceneView scene;
  const int* seeds; int nSeeds;     // launch seeds, one sample per pixel each (device memory)
  float* accum;                     // accuBuffer: float3 W*H, row 0 = bottom
  float* sampleBuf;                 // per-sample results: float3 [nSeeds][nItems]
  int* workCounter;                 // [0] global work-item counter, [1] watchdog flag (both zeroed before the launch); variant 4: the drain list behind them (kDrain*)
  int nItems;                       // pixels-slots of this rank = local tiles * 64
  int nWork;                        // work items = nSeeds * nItems, item k = (sample k / nItems, slot k % nItems)
  int tilesX; int rank, nRanks;     // 8x8 tile grid + tile-interleaved partition
  int exitThreshold;                // leave the traversal loop below this many active lanes
  int leafThreshold;                // run the leaf pass once this many lanes are parked at a leaf
  int* stackOverflow;               // per-thread spill area for trees deeper than the LDS stack (or null)
  unsigned long long* counters;     // kCntTotal x u64, laid out by pt_counters.h (counting build only)
  // variants 3 and 4 (queuekernel.hip, packetkernel.hip)
  void* poolCold;                   // path-slot records in HBM
  int starveLanes;                  // run a partial batch once this many lanes of the wave have nothing to traverse
  int swapLanes;                    // leave the node loop once this many lanes stand at a leaf / have finished
  int ovfDepth;                     // ints of stack overflow per slot
  int slotsInUse;                   // path slots per pool a launch uses (0 = all); fewer slots = shorter critical path
  int auxDepth;                     // variant 4: paths this deep trace their shadow rays in borrowed slots, beside the continuation (0 = off)
  unsigned long long watchdogTicks; // a wave gives up after this many 100 MHz ticks (sets workCounter[1]; the pass is then not reduced)
  // hand-out order of the work items (queuekernel.hip): tile-major, tiles with the deepest paths first
  int tileMajor;                    // 0 = sample-major in raster tile order (item k handed out as k); 1, 2 = by tile; 3 = by pixel
  int unitShift;                    // log2 of the slots per history unit: 6 = 8x8 tile, 0 = pixel
  const int* tileOrder;             // unit visited i-th (device, nItems >> unitShift entries) or nullptr = raster order
  unsigned int* tileCost;           // per unit: deepest path seen so far (device) or nullptr
#ifdef PT_EVLOG
  unsigned long long* evLog;        // experiment build (packetkernel.hip PT_EV): [0] events so far, [1..] the events
#endif
};
constexpr int kDeepPath = 8;        // paths at least this deep are recorded in tileCost
constexpr int kDrainDeep = 24;      // paths at least this deep go to the front of the drain list
// The launch's last paths (packetkernel.hip -> drainkernel.hip): a workgroup of the packet kernel that is down to `below` paths hands each of them
// over at its next packet boundary -- the slot record in poolCold is complete then -- and leaves.  The list lives behind the work counter
// (LaunchArgs::workCounter + kDrainList) and NOT in LaunchArgs: sixteen more bytes of kernel arguments moved the packet kernel's register
// allocation and cost 0.8 % of the benchmark frame (NOTEBOOK.md round 6).
//   [kDrainDeepN] deep paths handed over (entries upwards from kDrainEntries), [kDrainNext] the drain kernel's hand-out counter,
//   [kDrainOtherN] the other paths (entries downwards from kDrainEntries + cap - 1), [kDrainCap] entries the list holds (workgroups x below),
//   [kDrainBelow] the threshold (0 = off); an entry = the path's slot record, as an index into poolCold
constexpr int kDrainList = 2, kDrainDeepN = 0, kDrainNext = 1, kDrainOtherN = 2, kDrainCap = 4, kDrainBelow = 5, kDrainEntries = 6;

// work item k -> (sample index, pixel).  Slot i = k % nItems is the (i & 63)-th pixel of this
// rank's (i >> 6)-th 8x8 tile.  Tiles are dealt to the ranks in raster order, nRanks at a time, and the deal
// rotates by one rank from each group of nRanks tiles to the next (tile-interleaved multi-GPU partition,
// SURVEY 8e): a plain t % nRanks gives every rank the same columns in every row when nRanks divides the
// tiles of a row (1920 / 8 = 240 tiles, 8 ranks), and the ranks' ray counts then differ by 3-4 %.
// False for pixels outside the frame (this includes the tiles past the end of a rank's last group).
PT_HD bool item_to_pixel(const LaunchArgs& a, int k, int& sample, int& pixel) {
  sample = k / a.nItems;
  const int i = k - sample * a.nItems;
  const int lt = i >> 6, in = i & 63;
  const int gt = lt * a.nRanks + (a.rank + lt) % a.nRanks;
  const int tx = gt % a.tilesX, ty = gt / a.tilesX;
  const int x = tx * 8 + (in & 7), y = ty * 8 + (in >> 3);
  pixel = y * a.scene.width + x;
  return (x < a.scene.width) & (y < a.scene.height);
}
// Hand-out index k -> canonical work item (the index item_to_pixel and the per-sample buffer use).  Tile-major:
// all samples of a tile are handed out back to back, tile after tile in tileOrder; the paths that bounce 256 times
// (a chain of ~1000 dependent rays, ~28 ms) then start early and overlap the bulk instead of forming the tail.
PT_HD int handout_to_item(const LaunchArgs& a, int k) {
  if (!a.tileMajor) return k;
  if (a.tileMajor == 3) {                               // all samples of a pixel back to back, deepest pixels first
    const int ui = k / a.nSeeds, sample = k - ui * a.nSeeds;
    return sample * a.nItems + (a.tileOrder ? a.tileOrder[ui] : ui);
  }
  const int per = a.nSeeds << 6;                       // items of one tile
  const int ti = k / per, r = k - ti * per;
  const int lt = a.tileOrder ? a.tileOrder[ti] : ti;
  if (a.tileMajor == 2) {                               // experiment: consecutive items = samples of ONE pixel
    const int in = r / a.nSeeds, sample = r - in * a.nSeeds;
    return sample * a.nItems + (lt << 6) + in;
  }
  return (r >> 6) * a.nItems + (lt << 6) + (r & 63);
}
// The two functions above in one, for the lean packet kernel (packetkernel_body.h, F == 0): hand-out index k -> work item, sample, pixel.
// handout_to_item knows the sample and the slot (tile, pixel in the tile) before it folds them into the item, and item_to_pixel has x and
// y before it folds them into the pixel: carried along, the divisions that recover them (by nItems on the tile-major paths, by the
// frame's width in begin_sample) are not made, and one rank skips the deal's rotation.  Same items, same pixels: a slot is below nItems on
// every path (k < nWork; an order list holds units of this rank), so item / nItems and item % nItems are the sample and the slot.
//
// The divisions that remain divide by launch constants: the first divisor of the hand-out (handout_divisor), the tiles of a row and, with
// more than one rank, the ranks.  Each is a multiplication and a shift by a pair the host computes once (magic_div):
//   for a divisor d in [1, 2^31) let l = ceil(log2 d), shift = 31 + l, mul = ceil(2^shift / d).  Then mul * d = 2^shift + e with 0 <= e < d <= 2^l,
//   and for a dividend 0 <= n < 2^31:  n * mul / 2^shift = n / d + n * e / (d * 2^shift), where n * e < 2^31 * 2^l = 2^shift, so the second
//   term is below 1 / d -- too small to carry n / d (whose fraction is at most (d - 1) / d) to the next integer: floor(n * mul / 2^shift) =
//   floor(n / d).  2^(l - 1) < d gives mul <= 2^32 - 1 for d > 1 (mul = 2^31 for d = 1): mul is a 32-bit word, and n * mul < 2^63 is an
//   unsigned 64-bit product.  (A 32-bit high product alone will not do: d = 1 needs shift = 31.)
// Every dividend here is a hand-out index below nWork, a tile number or rank + tile number: non-negative ints, which plan_launch keeps below 2^31.
// The pairs are not kernel arguments (sixteen more bytes of those cost 0.8 %, above): they sit in FRONT of the work counter, at
// workCounter[-kHandoutWords ..], where the host writes them with the rest of the work header, and are read by scalar loads where they are used.
struct MagicDiv { unsigned int mul, shift; };
struct HandoutConsts { MagicDiv first, tilesX, ranks, seeds; };      // seeds: "tile_major" 2 alone divides by nSeeds a second time
constexpr int kHandoutWords = 8;
static_assert(sizeof(HandoutConsts) == kHandoutWords * sizeof(int), "HandoutConsts is kHandoutWords ints");
inline MagicDiv magic_div(int d) {
  int l = 0;
  while ((1ll << l) < (long long)d) l++;
  MagicDiv m; m.shift = 31u + (unsigned int)l;
  m.mul = (unsigned int)(((1ull << m.shift) + (unsigned long long)d - 1ull) / (unsigned long long)d);
  return m;
}
PT_HD int magic_quot(int n, MagicDiv m) { return (int)(((unsigned long long)(unsigned int)n * (unsigned long long)m.mul) >> m.shift); }
// what the hand-out divides k by first: the work items of a sample, of a pixel or of a tile
inline int handout_divisor(int tileMajor, int nItems, int nSeeds) { return !tileMajor ? nItems : tileMajor == 3 ? nSeeds : nSeeds << 6; }
inline HandoutConsts handout_consts(int tileMajor, int nItems, int nSeeds, int tilesX, int nRanks) {
  HandoutConsts h;
  h.first = magic_div(handout_divisor(tileMajor, nItems, nSeeds)); h.tilesX = magic_div(tilesX); h.ranks = magic_div(nRanks); h.seeds = magic_div(nSeeds);
  return h;
}

struct WorkItem { int item, sample, x, y, pixel; };
PT_HD bool handout_lean(const LaunchArgs& a, const HandoutConsts* hc, int k, WorkItem& w) {      // each pair is loaded where it is used: two scalar registers, briefly
  int slot;
  const int q = magic_quot(k, load_uniform(&hc->first));      // k / (nItems | nSeeds | nSeeds << 6)
  if (!a.tileMajor) {
    w.sample = q; slot = k - q * a.nItems;
  } else if (a.tileMajor == 3) {
    w.sample = k - q * a.nSeeds;
    slot = a.tileOrder ? a.tileOrder[q] : q;
  } else {
    const int r = k - q * (a.nSeeds << 6);
    const int lt = a.tileOrder ? a.tileOrder[q] : q;
    int in;
    if (a.tileMajor == 2) { in = magic_quot(r, load_uniform(&hc->seeds)); w.sample = r - in * a.nSeeds; }
    else { w.sample = r >> 6; in = r & 63; }
    slot = (lt << 6) + in;
  }
  w.item = a.tileMajor ? w.sample * a.nItems + slot : k;
  const int lt = slot >> 6, in = slot & 63;
  int gt = lt;
  if (__builtin_expect(a.nRanks != 1, 0)) { const int s = a.rank + lt; gt = lt * a.nRanks + (s - magic_quot(s, load_uniform(&hc->ranks)) * a.nRanks); }
  const int ty = magic_quot(gt, load_uniform(&hc->tilesX)), tx = gt - ty * a.tilesX;
  w.x = tx * 8 + (in & 7); w.y = ty * 8 + (in >> 3);
  w.pixel = w.y * a.scene.width + w.x;
  return (w.x < a.scene.width) & (w.y < a.scene.height);
}
#if defined(__HIPCC__)
// Camera.cu:39 result of one sample; Camera.cu:41 (the add) happens in k_reduce_samples
__device__ __forceinline__ void store_sample(const LaunchArgs& a, int item, v3 value) {
  float* sp = a.sampleBuf + 3 * (size_t)item;
  sp[0] = value.x; sp[1] = value.y; sp[2] = value.z;
}
#endif

// Which build of the packet kernel (packetkernel.hip) a launch runs.  General: every FEAT_* program (pt_types.h), counting and fast shading.
// Aux and Slim are the lean builds -- no optional program, uncounted, exact shading -- with borrowed slots and glass (Aux) or without (Slim).
// sceneFeatures: the FEAT_* programs the scene can reach, from the host's tables (api_core.hip scene_features; FEAT_ALL = do not specialise).
// slimEligible: the plan rules out borrowed slots (LaunchArgs::auxDepth == 0) and, for a scene whose shadow rays do not keep their nearest
// candidate, a Disney GLASS material.  Neither is a kernel argument: sixteen bytes of arguments cost the packet kernel 0.8 % (the drain list, above).
enum class PacketBuild { General, Aux, Slim };      // General = 0: what a zeroed LaunchPlan holds, and what every other trace kernel is handed
inline PacketBuild packet_build(bool counted, bool fastShading, int sceneFeatures, bool slimEligible) {
  if (counted || fastShading || sceneFeatures != 0) return PacketBuild::General;
  return slimEligible ? PacketBuild::Slim : PacketBuild::Aux;
}

int megakernel_lds_stack_entries();
hipError_t launch_reduce_samples(hipStream_t stream, const LaunchArgs& a);
hipError_t launch_megakernel(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted);
int queuekernel_lds_stack_entries();
int queuekernel_slots();
size_t queuekernel_cold_bytes(int nBlocks);
size_t queuekernel_overflow_ints(int nBlocks, int ovfDepth);
hipError_t launch_queuekernel(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild);
// queuekernel_lean.hip: the same kernel with four workgroups per CU, for scenes without triangles
int queuekernel_lds_stack_entries_lean();
int queuekernel_slots_lean();
size_t queuekernel_cold_bytes_lean(int nBlocks);
size_t queuekernel_overflow_ints_lean(int nBlocks, int ovfDepth);
hipError_t launch_queuekernel_lean(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild);
int packetkernel_lds_stack_entries();
int packetkernel_slots();             // path slots per workgroup (variant 4)
size_t packetkernel_cold_bytes(int nBlocks);
size_t packetkernel_overflow_ints(int nBlocks, int ovfDepth);
hipError_t launch_packetkernel(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild build);      // build: packet_build of the same counted, fastShading
// What the launch plan (api_render.hip) asks of a trace kernel that keeps its paths in slots: the stack entries a slot has in LDS, the bytes of
// slot records and the ints of stack overflow that nBlocks workgroups need, and the launch itself.  (launch_megakernel has no slots and sizes
// its overflow area per thread: it stays a special case there.)
struct TraceKernel {
  const char* launchWhat;
  int (*lds_stack_entries)();
  size_t (*cold_bytes)(int nBlocks);
  size_t (*overflow_ints)(int nBlocks, int ovfDepth);
  hipError_t (*launch)(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild build);      // build: the packet kernel's alone
};
inline constexpr TraceKernel kQueueKernel = { "launch queue megakernel", queuekernel_lds_stack_entries, queuekernel_cold_bytes, queuekernel_overflow_ints, launch_queuekernel };
inline constexpr TraceKernel kLeanQueueKernel = { "launch queue megakernel (lean)", queuekernel_lds_stack_entries_lean, queuekernel_cold_bytes_lean, queuekernel_overflow_ints_lean, launch_queuekernel_lean };
inline constexpr TraceKernel kPacketKernel = { "launch packet megakernel", packetkernel_lds_stack_entries, packetkernel_cold_bytes, packetkernel_overflow_ints, launch_packetkernel };
// drainkernel.hip: finishes the paths the packet kernel's workgroups handed over (LaunchArgs::drainList); same stream, right after it
hipError_t launch_drainkernel(hipStream_t stream, const LaunchArgs& a, int nCUs, bool counted, bool fastShading);
size_t drain_list_ints(int nBlocks, int drainBelow);      // ints behind LaunchArgs::workCounter + kDrainList
hipError_t launch_debug_trace(hipStream_t stream, const SceneView& sc, const float* dRays, int n, float* dT, int* dPrim, int* stackOverflow);
// node steps and triangle tests of one sample per pixel of sc.width x sc.height, paths cut at depth 6, under one node format
// (dOut[0..1] += ; megakernel.hip k_probe_paths)
hipError_t launch_probe_paths(hipStream_t stream, const SceneView& sc, int launchSeed, bool node64, unsigned long long* dOut, int* stackOverflow);
hipError_t launch_resolve_rgb8(hipStream_t stream, float* accum, int width, int height, float nAccumulation, int clearBuffer, uint8_t* dOut);

}  // namespace pt
