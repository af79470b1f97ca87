// pt_slotio.h -- how the slot kernels move the 16-byte rows of a path-slot record (queuekernel.hip's SlotCold, pt_slot.h's): the row of four ints
// and the load / store every row goes through.
#pragma once
#include "pt_types.h"

namespace pt {
namespace {

struct alignas(16) i4 { int x, y, z, w; };

// Slot records stream through the cache hierarchy once per visit; PT_SLOT_NT marks their loads/stores
// non-temporal so that they do not push BVH nodes out of the 4 MB L2 of the XCD.
#ifndef PT_SLOT_NT
#define PT_SLOT_NT 0
#endif
typedef float f4v __attribute__((ext_vector_type(4)));
template <class T> __device__ __forceinline__ T slot_load(const T* p) {
  static_assert(sizeof(T) % 16 == 0, "16-byte granules");
  if constexpr (PT_SLOT_NT) {
    T out;
    const f4v* src = reinterpret_cast<const f4v*>(p); f4v* dst = reinterpret_cast<f4v*>(&out);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) dst[i] = __builtin_nontemporal_load(src + i);
    return out;
  } else {
    return *p;
  }
}
template <class T> __device__ __forceinline__ void slot_store(T* p, const T& v) {
  static_assert(sizeof(T) % 16 == 0, "16-byte granules");
  if constexpr (PT_SLOT_NT) {
    const f4v* src = reinterpret_cast<const f4v*>(&v); f4v* dst = reinterpret_cast<f4v*>(p);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) __builtin_nontemporal_store(src[i], dst + i);
  } else {
    *p = v;
  }
}

}  // namespace
}  // namespace pt
