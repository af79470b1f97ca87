// packetkernel.hip -- megakernel variant 4: the scheduler of variant 3 (queuekernel.hip: path slots with their traversal
// state in LDS, node / leaf / shade / gen queues shared by the workgroup, lanes as workers) around the PER-BOUNCE state
// machine of pt_packet.h.  What the two schedulers declare alike (workgroup shape, queue ids, wave rings, slot stack, fresh_args) is in pt_sched.h.
//
// Variant 3 gives every ray its own shading visit: a Disney hit with three facing lights is four trips through the
// shade queue, four slot-record round trips and four traversal set-ups, one after the other.  Here a visit does all of a
// hit's work that does not depend on a trace (every light draw, the facing tests, disneyPdf / disneyEval per light, the
// BRDF sample, the seed fork) and leaves a PACKET: up to three shadow rays and the continuation ray, all from the hit
// point.  The slot then traces the packet's rays one after the other WITHOUT going back to shading: when a ray ends and
// another one is pending, the next leaf pass -- or, in a kernel built with SWITCH (below), the scheduler loop itself where the ray
// ended in the node loop -- loads that ray (16 bytes of the slot record) and restarts the slot at the root.  The visit that follows folds the shadow results into the radiance in light order and shades the continuation's
// hit.  Same random draws, same decisions, same floating-point operations on the path's values as variants 0-3 (the
// images are bit-identical); a path of depth k is a chain of k visits instead of up to 4k.
//
// Deep paths (LaunchArgs::auxDepth) go one step further: the shadow rays of a hit are traced in slots BORROWED from
// finished paths, at the same time as the continuation, and joined through three bits of the path slot's LDS flag word
// (see PoolLds::freeMask, SlotSink, store_flags / arrive_parks / aux_done).  A launch's tail is a handful of paths
// walking the 256-bounce cap; this makes each of their bounces one dependent ray instead of up to four.
//
// What a pass touches (round 4):
//   * a finished packet is routed by what its continuation hit (kShadeFlag): Disney triangle hits to Q_SHADE, whose batches run the
//     Disney program on full waves, everything else to Q_GEN, whose visit also takes the next work item;
//   * the leaf pass makes ONE memory round trip: triangle records only -- no hit row (a tie at exactly tbest reads it), no material
//     (Tri48::shadow says what a triangle is to a shadow ray), the packet's next ray only where this ray can end;
//   * shade batches and leaf passes read the launch arguments through fresh_args(): nothing of the scene sits in scalar
//     registers while the node loop runs;
//   * 576 path slots x 9 LDS stack entries per workgroup: rings sized exactly, 53,104 of the 53,760 bytes three workgroups per CU get.
//
//   * round 6: a workgroup that is down to its last paths (the launch's drain) stops shading partial batches and, once every path it has left waits in
//     Q_SHADE / Q_GEN, hands them to drainkernel.hip BEHIND the main loop and leaves (the block after the loop says why it is there and not in it);
//   * round 22: a third compile-time switch of the body, SWITCH, beside AUX and GLASS (all three are described in front of the kernels below): the
//     NEAR = false slim kernels take a packet's next ray up in the scheduler loop's leave handler where a ray ends in the node loop, and their leaf
//     pass has no switch arm; every other kernel keeps the hop through the leaf ring (kSwitchRef);
//   * round 24: DIET, four 4.3-clock vector instructions per node step taken out of the slim kernels at compile time (in front of the kernels below);
//   * this file is compiled twice (Makefile): as it stands for the 64-byte-node instantiations, with LLVM's max-ilp scheduling, and through
//     packetkernel_n128.hip (PT_PK_N128) for the 128-byte-node ones with the default strategy -- each is a few per cent slower under the other's.
//
// Limits (api_render.hip plan_launch falls back to variant 3 otherwise): at most kPacketShadows lights, no Disney material on an
// analytic primitive (shadow rays then need the brute-force lists at every ray start).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "megakernel.h"
#include "pt_lanestack.h"
#include "pt_path.h"
#include "pt_packet.h"
#include "pt_sched.h"
#include "pt_slot.h"

namespace pt {

namespace {

// Path slots per wave and LDS stack entries per slot: what a workgroup's third of the CU's LDS (53,760 bytes for three workgroups:
// 42 blocks of 1,280; a 54,128-byte build ran two per CU) is spent on.  A slot costs 32 B of ray + 4 (entries + 1) B of stack + 12 B of ring space.  Measured on
// coffee at 64 spp, same bits (profiles/r04_slots.txt): 512 slots x 11 entries 95.3 ms, 544 x 10 93.8, 576 x 9 93.3, 608 x 8 93.9,
// 640 x 7 94.5 -- more paths in flight against more stack entries spilled to HBM.  (queuekernel.hip keeps its own 512 x 11.)
#ifndef PT_PK_KP
#define PT_PK_KP 144
#endif
#ifndef PT_PK_STACKN
#define PT_PK_STACKN 9
#endif
#define PT_KP PT_PK_KP
#define PT_STACKN PT_PK_STACKN
#ifndef PT_WAVES_PER_SIMD
#define PT_WAVES_PER_SIMD 3
#endif
constexpr int kP = PT_KP;               // slots per wave
constexpr int kStackN = PT_STACKN;      // LDS stack entries per slot; deeper levels spill to HBM
constexpr int kWavesPerSimd = PT_WAVES_PER_SIMD;   // occupancy target: 3 workgroups per CU (VGPR <= 168, LDS <= 53 KB)
// Rings hold exactly NS entries (a slot sits in at most one ring): sized to the next power of two they would cost 640 -> 1024
// entries each and the workgroup its third of the CU's LDS.  An index is head + count + rank < 2 NS: one conditional subtract.
template <int NS> __device__ __forceinline__ int ring_wrap(int i) {
  if constexpr ((NS & (NS - 1)) == 0) return i & (NS - 1); else return i >= NS ? i - NS : i;
}
static_assert(PT_KP * kWaves <= (1 << kSlotBits), "slot ids are 10 bits");

// LDS image of NS slots
template <int NS>
struct PoolLds {
  // only what the node loop touches lives in LDS: 32 B + the stack per slot
  v4 nodeA[NS];           // o.xyz, tbest
  v4 nodeB[NS];           // d.xyz, node (int bits); a lane that picks the slot up for the node loop derives 1/d from it
  int stack[NS][kStackN + 1];   // [0] = sp | packet description (see the flag bits below), [1..] = entries
  unsigned short queue[kNumQ][NS];
  int qHead[kNumQ], qCount[kNumQ];
  int done, lock;
  int drainAt;                       // once this many slots are done the pool stops shading and hands its last paths to the drain kernel (set at start-up)
  // Concurrent shadow rays for deep paths (LaunchArgs::auxDepth): a slot whose path is done (the work items ran out, or
  // LaunchArgs::slotsInUse left it without one) can be borrowed by a deep path, one per shadow ray of a hit, so that
  // the shadow rays and the continuation are traced at the same time: the launch's tail is a few capped paths walking
  // their 257 bounces, and this divides the time each bounce takes.
  unsigned int freeMask[NS / 32];    // bit set: the slot carries no path and nobody has borrowed it
  int nFree;                         // set bits in freeMask (approximate: read without the lock)
};

typedef __attribute__((address_space(3))) volatile f4v lds_volatile_f4v;      // a 16-byte LDS store the compiler neither merges nor splits (packetkernel_body.h, SWITCH)

using SlotStack = LdsStack<kStackN, true>;      // pt_path.h node_step_nearfar: this stack takes the branch-free tail

// pt_packet.h's sink for the shadow rays of a new packet: each goes to the slot as soon as it is known (weight row; the ray
// itself to LDS if it is the first of the list, else to its ray row) -- or, for a deep path that has borrowed slots, each
// shadow ray goes to its own borrowed slot, to be traced at the same time as the continuation.
struct SlotSink {
  SlotCold* cold; int slot; v4* nodeA; v4* nodeB; int (*stack)[kStackN + 1]; const PathState* ps; int root;
  int axp;                              // this path's three borrowed slots (10 bits each) or -1
  __device__ __forceinline__ void shadow(int j, v3 d, float tmax, v3 w, float inv) const {
    SlotCold* cw = at32(cold, slot);
    slot_store(&cw->pend[j], mk4(w.x, w.y, w.z, inv));
    if (axp >= 0) {
      const int ax = (axp >> (kSlotBits * j)) & kSlotMask;
      nodeA[ax] = mk4(ps->o.x, ps->o.y, ps->o.z, tmax); nodeB[ax] = mk4(d.x, d.y, d.z, i2f(root));
      stack[ax][0] = kAuxSlot | kShadowRay | (1 << kNShShift) | aux_parent_bits(slot);      // a packet of one shadow ray
    } else if (j == 0) { nodeA[slot] = mk4(ps->o.x, ps->o.y, ps->o.z, tmax); nodeB[slot] = mk4(d.x, d.y, d.z, i2f(root)); }   // ps->o: the hit point
    else slot_store(&cw->ray[j - 1], mk4(d.x, d.y, d.z, tmax));
  }
};

// The same sink for a kernel without borrowed slots (AUX = false, below): no `axp` to carry through the Disney visit.
struct OwnSlotSink {
  SlotCold* cold; int slot; v4* nodeA; v4* nodeB; const PathState* ps; int root;
  __device__ __forceinline__ OwnSlotSink(SlotCold* cold_, int slot_, v4* nodeA_, v4* nodeB_, int (*)[kStackN + 1], const PathState* ps_, int root_, int /*axp*/)
      : cold(cold_), slot(slot_), nodeA(nodeA_), nodeB(nodeB_), ps(ps_), root(root_) {}
  __device__ __forceinline__ void shadow(int j, v3 d, float tmax, v3 w, float inv) const {
    SlotCold* cw = at32(cold, slot);
    slot_store(&cw->pend[j], mk4(w.x, w.y, w.z, inv));
    if (j == 0) { nodeA[slot] = mk4(ps->o.x, ps->o.y, ps->o.z, tmax); nodeB[slot] = mk4(d.x, d.y, d.z, i2f(root)); }   // ps->o: the hit point
    else slot_store(&cw->ray[j - 1], mk4(d.x, d.y, d.z, tmax));
  }
};

// NEAR: the scene has a Disney GLASS material, shadow rays keep their nearest any-hit candidate (pt_path.h, rule D5).  A template
// parameter so that scenes without one -- the benchmark scene -- run code in which that logic does not exist.
// F (pt_types.h FEAT_*): the programs the per-lane code of a kernel contains.  The same reasoning one step further: this kernel's
// register allocation reacts to code its loop never executes (NOTEBOOK.md rounds 4-6), and a scene of untextured Disney meshes under quad
// lights -- the benchmark scene -- cannot reach the texture path (three double-precision pow() expansions), the sphere-light draw, the
// Lambertian / metal / glass programs or the analytic sphere loops.
//
//
// AUX, GLASS (round 21): two more things a launch can rule out, compile-time switches of the body and no FEAT_* bits.  AUX = false: the launch
// borrows no slots (LaunchArgs::auxDepth 0 -- what plan_launch gives a launch of 1e8 samples or more, which keeps no slot free to borrow) and
// the kernel holds none of that machinery: no `axp` live across the Disney visit, no join test in the leaf pass and the leave handler, no
// claim loop in the batch store.  GLASS = false: no material is Disney GLASS, so a shadow ray's attenuation is (1,1,1) or (0,0,0): no
// tinted `att` rows in the leaf pass and the batch load, no material id kept per leaf triangle.  A NEAR kernel always has GLASS.
// The Disney program's glass arm (pt_path.h on_result -> glass_body) STAYS in every build: compiled out as well, the timed kernel took all
// 168 vector registers and 28 spilled scalar ones (with it: 148 and 21; its twin: 159 and 25) for 0.85 ms of a 291 ms frame, which is
// no gain by the project's rule (profiles/r21_slim_ab.txt), and tests/test_packet_resources_cpu.py holds the slim kernels to their twins' numbers.
//
// Three __global__ templates, one body.  The SLIM kernel (no FEAT_* bit, AUX = false, GLASS = NEAR: what the benchmark frame runs) keeps the
// name the kernel has had since round 3 -- the profiles, tools/kernel_resources.py listings and the resource pin of the timed instantiation
// go by it.  pt_packetkernel_aux is the lean kernel of rounds 19-20 (no FEAT_* bit, borrowed slots, glass): lean launches that borrow slots
// (short launches, "aux_depth" with "slots_in_use") or meet glass under "shadow_rule" 0.  The kernel that contains every program is
// pt_packetkernel_general.  The body is packetkernel_body.h, included into each as
// their own statements: behind a call, even a forced-inline one, the general kernels came out with other register numbers and another
// instruction order than they have had (same spill counts; the glass knot ran 0.75 % slower, NOTEBOOK.md round 19, as round 18 had found
// for the point kernels).  Included, they are the parent's instruction for instruction.
// -DPT_PK_SLIM_GLASS / -DPT_PK_SLIM_AUX (experiment builds, profiles/r21_slim_ab.txt): the slim kernel with one switch alone.
#ifdef PT_PK_SLIM_GLASS
constexpr bool kSlimKeepsGlass = true;
#else
constexpr bool kSlimKeepsGlass = false;
#endif
#ifdef PT_PK_SLIM_AUX
constexpr bool kSlimKeepsAux = true;
#else
constexpr bool kSlimKeepsAux = false;
#endif
// SWITCH (round 22): where a packet's next ray is taken up when a ray ends in the NODE LOOP (a step that enters no child with an empty stack: an
// unoccluded shadow ray, a miss).  false: the lane leaves the slot at kSwitchRef on the leaf ring and a whole leaf pass carries it, only to load
// one ray row.  true: the leave handler requests that row itself, the load travels while the wave runs its next pass, and the top of the next
// scheduler iteration puts the slot back on the wave's node ring; the leaf pass then holds no switch arm at all.  Slim kernels only: a switch
// needs the plain flag-word store of AUX = false, and the twins and the general kernels stay what they were.  And of the slim kernels only the
// two with NEAR = false: the row and the slot id are five vector registers alive through the Disney visit, which take the NEAR kernels two
// registers past their twins (161 / 160 against 159 / 158; tests/test_packet_resources_cpu.py holds them to the twins' numbers), so those keep the hop.
// -DPT_PK_SWITCH_LEAF (experiment build, profiles/r22_switch_ab.txt): the slim kernels with the switch in the leaf pass, as before round 22.
#ifdef PT_PK_SWITCH_LEAF
constexpr bool kSlimSwitches = false;
#else
constexpr bool kSlimSwitches = true;
#endif
// -DPT_PK_SWITCH_ARM (experiment build): the leave handler switches, and the leaf pass keeps the arm nothing reaches -- the first step alone.
#ifdef PT_PK_SWITCH_ARM
constexpr bool kLeafKeepsSwitchArm = true;
#else
constexpr bool kLeafKeepsSwitchArm = false;
#endif
// DIET (round 24): four 4.3-clock vector instructions per node step that the slim launch cannot need, taken out at compile time.  All four slim kernels
// have it (their pins hold, profiles/r24_kernel_resources.txt); the twins and the general kernels do not and stay what they were.
//   * the node loop's header finds the lanes at a node by ONE compare whose scalar register pair is the lane mask (the ballot of the three-part
//     bool was a 0 / 1 select and a second compare, two 4.3-clock instructions per node step);
//   * the slab test takes tmin and tbest into single v_max_f32 / v_min_f32 (pt_path.h lean_max / lean_min) where the compiler put a canonicalising
//     v_max_f32 x, x in front of each, every step, because it cannot see that a kernel argument and an LDS word are not signalling NaNs.
// Coffee 287.08 -> 282.61 ms (profiles/r24_diet_ab.txt).  Two more groups were built and measured on top and are NOT in the code, being no gain by
// the project's rule (+0.2 to +0.3 ms, inside the spread): a leaf pass of one chunk for trees with leaves of at most four triangles, and the lens
// sample's rejection test on the squared length (NOTEBOOK.md round 24).
// -DPT_PK_NO_DIET_NODE (experiment build): the slim kernels of round 23, instruction for instruction.
#ifdef PT_PK_NO_DIET_NODE
constexpr bool kSlimDietNode = false;
#else
constexpr bool kSlimDietNode = true;
#endif
// tmin reaches the slab test's v_max_f32 through a vector register: one v_mov_b32 per step, and a v_readlane_b32 where its scalar register is a spilled one.  As the instruction's scalar operand it needs none
// and was SLOWER: coffee 283.89 ms against 281.76 (parent 286.21; profiles/r24_diet_ab.txt), with one spilled scalar register more in every slim
// kernel -- in the 128-byte-node NEAR = false one 19, past its twin's 18 (tests/test_packet_resources_cpu.py).  That form is not kept.
using DietStack = LdsStack<kStackN, true, true>;      // pt_path.h node_step_nearfar, stack_diet: lean_max / lean_min for tmin and tbest
template <bool CNT, bool SHARED, bool FAST = false, bool NEAR = false, bool N64 = false>
__global__ void __launch_bounds__(kBlockThreads, kWavesPerSimd) pt_packetkernel(const LaunchArgs a) {
  constexpr int F = 0;
  constexpr bool AUX = kSlimKeepsAux, GLASS = NEAR || kSlimKeepsGlass, SWITCH = kSlimSwitches && !kSlimKeepsAux && !NEAR;
  constexpr bool DIET_NODE = kSlimDietNode && !AUX;
#include "packetkernel_body.h"
}
template <bool CNT, bool SHARED, bool FAST = false, bool NEAR = false, bool N64 = false>
__global__ void __launch_bounds__(kBlockThreads, kWavesPerSimd) pt_packetkernel_aux(const LaunchArgs a) {
  constexpr int F = 0;
  constexpr bool AUX = true, GLASS = true, SWITCH = false;
  constexpr bool DIET_NODE = false;
#include "packetkernel_body.h"
}
template <bool CNT, bool SHARED, bool FAST = false, bool NEAR = false, bool N64 = false>
__global__ void __launch_bounds__(kBlockThreads, kWavesPerSimd) pt_packetkernel_general(const LaunchArgs a) {
  constexpr int F = FEAT_ALL;
  constexpr bool AUX = true, GLASS = true, SWITCH = false;
  constexpr bool DIET_NODE = false;
#include "packetkernel_body.h"
}

}  // namespace

// The instantiations are compiled in two translation units, by node format: this file holds the 64-byte-node kernels (the benchmark scene's), and
// packetkernel_n128.hip includes it with PT_PK_N128 for the 128-byte-node ones.  The reason is the compiler, not the code: LLVM's instruction
// scheduling strategy is a per-file flag (Makefile), "max-ilp" is 0.85 % faster than the default on the 64-byte kernels (coffee 312.5 -> 309.9 ms,
// glass knot -1.5 %) and 2-4 % SLOWER on the 128-byte ones (dining room) and on the queue kernels (random spheres) -- measured, round 6.
#ifndef PT_PK_N128
// Three builds exist per node format and shadow rule (megakernel.h PacketBuild): every program (FEAT_ALL) and none of the optional ones (0), the
// latter uncounted and with exact shading only, with borrowed slots and glass (_aux) or without (the slim build).  A scene that needs any one
// of the programs runs the general build.
int packetkernel_lds_stack_entries() { return kStackN; }
int packetkernel_slots() { return kP * kWaves; }
size_t packetkernel_cold_bytes(int nBlocks) { return (size_t)nBlocks * kWaves * kP * sizeof(SlotCold); }
size_t packetkernel_overflow_ints(int nBlocks, int ovfDepth) { return (size_t)nBlocks * kWaves * kP * (size_t)ovfDepth; }
constexpr bool kThisFileN64 = true;
#define PT_PK_LAUNCH launch_packetkernel_n64
#else
constexpr bool kThisFileN64 = false;
#define PT_PK_LAUNCH launch_packetkernel_n128
#endif

template <bool CNT, bool FAST>
static void launch_pk(dim3 grid, dim3 block, hipStream_t stream, const LaunchArgs& a) {
  if (a.scene.shadowNearest) pt_packetkernel_general<CNT, true, FAST, true, kThisFileN64><<<grid, block, 0, stream>>>(a);
  else                       pt_packetkernel_general<CNT, true, FAST, false, kThisFileN64><<<grid, block, 0, stream>>>(a);
}
hipError_t PT_PK_LAUNCH(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild build) {
  dim3 grid(nBlocks), block(kBlockThreads);
  switch (build) {
  case PacketBuild::Slim:      // lean, and the plan rules borrowed slots and (NEAR = false) glass out
    if (a.auxDepth != 0 && !kSlimKeepsAux) return hipErrorInvalidValue;                           // (the kernel would ignore it: the plan never asks for this)
    if (a.scene.shadowNearest) pt_packetkernel<false, true, false, true, kThisFileN64><<<grid, block, 0, stream>>>(a);
    else                       pt_packetkernel<false, true, false, false, kThisFileN64><<<grid, block, 0, stream>>>(a);
    break;
  case PacketBuild::Aux:       // lean: uncounted, exact shading
    if (a.scene.shadowNearest) pt_packetkernel_aux<false, true, false, true, kThisFileN64><<<grid, block, 0, stream>>>(a);
    else                       pt_packetkernel_aux<false, true, false, false, kThisFileN64><<<grid, block, 0, stream>>>(a);
    break;
  case PacketBuild::General:
    if (fastShading) { if (counted) launch_pk<true, true>(grid, block, stream, a); else launch_pk<false, true>(grid, block, stream, a); }
    else             { if (counted) launch_pk<true, false>(grid, block, stream, a); else launch_pk<false, false>(grid, block, stream, a); }
    break;
  }
  return hipGetLastError();
}
#ifndef PT_PK_N128
hipError_t launch_packetkernel_n128(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild build);
hipError_t launch_packetkernel(hipStream_t stream, const LaunchArgs& a, int nBlocks, bool counted, bool fastShading, PacketBuild build) {
  // api_core.hip fill_view: the option node_format decides whether the scene view carries the 64-byte nodes
  return a.scene.nodes64 != nullptr ? launch_packetkernel_n64(stream, a, nBlocks, counted, fastShading, build) : launch_packetkernel_n128(stream, a, nBlocks, counted, fastShading, build);
}
#endif

}  // namespace pt
