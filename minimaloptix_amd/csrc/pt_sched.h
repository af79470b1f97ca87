// pt_sched.h -- what the two scheduler kernels (queuekernel.hip, variant 3; packetkernel.hip, variant 4) declare alike: the workgroup's shape,
// the queue ids, a wave's private rings, a slot's traversal stack, the launch arguments afresh and the sub-phase clocks of the counting
// builds.  The slot records, the pools' LDS images, the passes and the main loops stay with each kernel: they look alike and are not (the
// register allocator treats them differently).
#pragma once
#include <hip/hip_runtime.h>

#include "megakernel.h"
#include "pt_slotio.h"

namespace pt {
namespace {

constexpr int kBlockThreads = 256;
constexpr int kWaves = kBlockThreads / 64;

// pool-wide queues first (they index PoolLds::queue); Q_NODE / Q_LEAF are per-wave rings (WavePriv)
enum { Q_SHADE = 0, Q_GEN = 1, kNumQ = 2, Q_NODE = 2, Q_LEAF = 3, DEST_DONE = 4, DEST_NONE = -1 };

// RC: the capacity of a ring that can hold every slot of the pool (the packet kernel sizes it exactly, the queue kernel to a power of two)
template <int RC>
struct WavePriv {
  unsigned short qnode[RC];        // node-ready slots owned by this wave (ring)
  // One loop iteration pushes at most 128 slots (results of the last pass + lanes leaving the node loop) to the rings below.  (Packet kernel,
  // SWITCH: the ray switches finished at the top of an iteration are 64 more, all to one ring: qnode, which has room for every slot -- or, in
  // a scene whose root is a leaf, qleaf, and then no lane ever walks the node loop, so none leaves it.)
  unsigned short qleaf[256];       // slots standing at a leaf, owned by this wave (ring; a pass runs at 64: < 64 + 128)
  unsigned short outbox[2][160];   // slots on their way to the pool's Q_SHADE / Q_GEN (flushed at 32: < 32 + 128)
};

typedef __attribute__((address_space(3))) int lds_int;

// A slot's traversal stack: STACKN entries in LDS, deeper levels in HBM.  The LDS part is addressed through an address_space(3) pointer
// so that push/pop compile to ds_write_b32/ds_read_b32 (a generic pointer makes the compiler merge the LDS and the HBM overflow path into
// one flat_load).
// FLAT: pt_path.h node_step_nearfar's branch-free tail -- m pushes on top of sp entries stay in LDS and entry sp exists (the dead store of a
// step that enters nothing lands there); the entry a pop would take (sp - 1; for sp = 0 the slot's flag word, unused).  Without it the stack
// takes the branched tail.
// DIET (packetkernel.hip, the slim kernels): the node step's slab test takes tmin and tbest without a canonicalising instruction (pt_path.h stack_diet).
template <int STACKN, bool FLAT, bool DIET = false>
struct LdsStack {
  lds_int* lds;           // &stack[slot][1]
  int* ovf;               // this slot's overflow area in HBM (or nullptr)
  __device__ __forceinline__ void store(int sp, int v) {
    if (__builtin_expect(sp < STACKN, 1)) lds[sp] = v; else ovf[sp - STACKN] = v;
  }
  __device__ __forceinline__ int load(int sp) const {
    int v;
    if (__builtin_expect(sp < STACKN, 1)) v = lds[sp]; else v = ovf[sp - STACKN];
    return v;
  }
  __device__ __forceinline__ bool roomy(int sp) const { return sp + 3 <= STACKN; }     // three pushes stay in LDS
  __device__ __forceinline__ void store_fast(int sp, int v) { lds[sp] = v; }
  static constexpr bool kFlat = FLAT;
  static constexpr bool kDiet = DIET;
  __device__ __forceinline__ bool fits_fast(int sp, int m) const { return FLAT && sp + m <= STACKN && sp < STACKN; }
  __device__ __forceinline__ int peek_fast(int sp) const { if constexpr (FLAT) return lds[min(sp, STACKN) - 1]; else return 0; }
};

// The launch arguments again, read from the kernel-argument segment through a pointer the compiler cannot see through.
// The kernel is one loop; whatever it reads from its arguments is loop-invariant, so the compiler loads ALL of it in front
// of the loop and keeps it in scalar registers for the whole launch: camera (19 words), background, a dozen table pointers,
// the hand-out parameters -- about 100 words against 102 registers, and the rest of the kernel's scalar state (queue heads,
// exec masks of the scheduler) then lives in lanes of a spill VGPR, one v_readlane / v_writelane (4.4 clocks of the vector
// pipe each, tools/micro/valu_issue.hip) per access: 111 spilled scalar registers in round 3 (the queue kernel shipped
// round 6 with 118-120).  A pass that needs the scene (shading batch, leaf pass) therefore takes its own copy here: s_load
// where the value is used, dead when the pass ends, and only what the node loop and the scheduler need stays resident.
__device__ __forceinline__ const LaunchArgs& fresh_args() {
  typedef __attribute__((address_space(4))) const LaunchArgs CA;
  unsigned long long p = (unsigned long long)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return *(const LaunchArgs*)(CA*)p;
}

// Sub-phase clocks of the counting build (CNT): PT_SUB0 starts the clock `tSub`, PT_SUB adds what has passed since to an accumulator;
// PT_STAMP does the same for the pass-level clock `tStamp`.  The kernel that uses them declares CNT, tSub and tStamp.
#define PT_SUB0() do { if (CNT) tSub = __builtin_amdgcn_s_memtime(); } while (0)
#define PT_SUB(acc) do { if (CNT) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - tSub; tSub = now_; } } while (0)
#define PT_STAMP(acc) do { if (CNT) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); acc += now_ - tStamp; tStamp = now_; } } while (0)

}  // namespace
}  // namespace pt
