// pt_word4.h -- what the sorted candidate lists of the multi-hit ray queries (pt_multihit.h) and the K-nearest point queries
// (pt_pointmulti.h) share: the 16-byte word their slices of the output are read and written as, and rule D5's order of two keys.
#pragma once
#include "pt_path.h"

namespace pt {

struct alignas(16) Word4 { uint32_t x, y, z, w; };
PT_HD Word4 mkw4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { Word4 r; r.x = x; r.y = y; r.z = z; r.w = w; return r; }

PT_HD bool key_less(float t, int prim, float tb, int primb) { return (t < tb) | ((t == tb) & (prim < primb)); }

}  // namespace pt
