// pt_pointstack.h -- the traversal stack of the kernels that walk a point query per lane (pointkernel.hip, signkernel.hip) and the shape
// of their workgroups.  Device code, for the .hip files only.
//
// The stack holds a child reference and the squared distance to its box side by side, eight bytes an entry: 16 entries per lane in LDS
// ([entry][lane], 32 KB per workgroup as the ray queries' 32 four-byte ones) with a global overflow column per thread.
#pragma once
#include "pt_lanestack.h"

namespace pt {

constexpr int kPointBlockThreads = 256;
constexpr int kPointWavesPerBlock = kPointBlockThreads / 64;
constexpr int kPointLdsStack = 16;          // entries per lane kept in LDS (8 bytes each: 32 KB per workgroup)

// LaneStack (pt_lanestack.h) over eight-byte entries: reference + box distance
struct PointStack : LaneStack<kPointLdsStack, unsigned long long> {
  __device__ __forceinline__ void store(int sp, int ref, float d2) {
    LaneStack::store(sp, ((unsigned long long)(uint32_t)f2i(d2) << 32) | (uint32_t)ref);
  }
  __device__ __forceinline__ void load(int sp, int& ref, float& d2) const {
    const unsigned long long e = LaneStack::load(sp);
    ref = (int32_t)(uint32_t)e; d2 = i2f((int32_t)(e >> 32));
  }
};

}  // namespace pt
