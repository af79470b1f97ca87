// devarith_ops.h -- the list of primitives of tests/devarith: one element-wise function per primitive of the arithmetic contract
// (pt_math.h AC1-AC7), each calling the product headers' own function.  The file is included twice: by devarith.hip, where DA_OP makes
// a kernel (one thread per element) and a table row, and by devarith_host.cpp, where it makes a loop compiled by the host compiler: the
// mirror side.  Same text, same headers; what differs is what the contract says may not matter.
//
// DA_OP(name, NIN, NOUT, body): body reads float x[NIN] and writes float y[NOUT].  Integers travel as their bits (f2i / i2f).
// DA_DEVICE_OP: a primitive that exists on the device alone (hardware approximations); the host table has no row for it.
#include "../../minimaloptix_amd/csrc/pt_path.h"
#include "../../minimaloptix_amd/csrc/pt_texture.h"
#include "../../minimaloptix_amd/csrc/pt_denoise.h"
#include "../../minimaloptix_amd/csrc/pt_sign.h"
#include "../../minimaloptix_amd/csrc/pt_rng.h"
#include "../../minimaloptix_amd/csrc/pt_disney.h"

// ---- AC4: single operations, as the headers write them
DA_OP(add, 2, 1, y[0] = x[0] + x[1];)
DA_OP(sub, 2, 1, y[0] = x[0] - x[1];)
DA_OP(mul, 2, 1, y[0] = x[0] * x[1];)
DA_OP(div, 2, 1, y[0] = x[0] / x[1];)
DA_OP(rcp, 1, 1, y[0] = 1.0f / x[0];)
DA_OP(sqrt, 1, 1, y[0] = __builtin_sqrtf(x[0]);)
DA_OP(fma, 3, 1, y[0] = pt::fma_(x[0], x[1], x[2]);)
DA_OP(floor, 1, 1, y[0] = floorf(x[0]);)
DA_OP(bfloor, 1, 1, y[0] = __builtin_floorf(x[0]);)
DA_OP(f2int, 1, 1, y[0] = pt::i2f((int)x[0]);)                        // defined for |x| < 2^31 only
DA_OP(int2f, 1, 1, y[0] = (float)(int)pt::f2i(x[0]);)                 // (float) of the int whose bits x carries
DA_OP(f2int2f, 1, 1, y[0] = (float)(int)x[0];)                        // tex2d's weight quantisation; |x| < 2^31
DA_OP(copysign, 2, 1, y[0] = __builtin_copysignf(x[0], x[1]);)
DA_OP(fabs, 1, 1, y[0] = __builtin_fabsf(x[0]);)
DA_OP(bits, 1, 1, y[0] = pt::i2f(pt::f2i(x[0]) ^ 0x55aa55aa);)        // f2i / i2f around an integer operation
DA_OP(rnd, 1, 2, uint32_t s = (uint32_t)pt::f2i(x[0]); y[0] = pt::rnd(s); y[1] = pt::i2f((int32_t)s);)
DA_OP(fmin, 2, 1, y[0] = pt::fminf_(x[0], x[1]);)
DA_OP(fmax, 2, 1, y[0] = pt::fmaxf_(x[0], x[1]);)
DA_OP(clamp, 3, 1, y[0] = pt::clampf(x[0], x[1], x[2]);)
DA_OP(lean_min, 2, 1, y[0] = pt::lean_min(x[0], x[1]);)
DA_OP(lean_max, 2, 1, y[0] = pt::lean_max(x[0], x[1]);)
DA_OP(lerp, 3, 1, y[0] = pt::lerp(x[0], x[1], x[2]);)
DA_OP(slab_inv, 1, 1, y[0] = pt::slab_inv(x[0]);)
// ---- AC1-AC3, AC7: the float3 forms
DA_OP(dot, 6, 1, y[0] = pt::dot(pt::mk3(x[0], x[1], x[2]), pt::mk3(x[3], x[4], x[5]));)
DA_OP(cross, 6, 3, const pt::v3 r = pt::cross(pt::mk3(x[0], x[1], x[2]), pt::mk3(x[3], x[4], x[5])); y[0] = r.x; y[1] = r.y; y[2] = r.z;)
DA_OP(length, 3, 1, y[0] = pt::length(pt::mk3(x[0], x[1], x[2]));)
DA_OP(normalize, 3, 3, const pt::v3 r = pt::normalize(pt::mk3(x[0], x[1], x[2])); y[0] = r.x; y[1] = r.y; y[2] = r.z;)
DA_OP(v3div, 4, 3, const pt::v3 r = pt::mk3(x[0], x[1], x[2]) / x[3]; y[0] = r.x; y[1] = r.y; y[2] = r.z;)
DA_OP(ray_at, 7, 3, const pt::v3 r = pt::ray_at(pt::mk3(x[0], x[1], x[2]), pt::mk3(x[3], x[4], x[5]), x[6]); y[0] = r.x; y[1] = r.y; y[2] = r.z;)
DA_OP(lerp3, 7, 3, const pt::v3 r = pt::lerp(pt::mk3(x[0], x[1], x[2]), pt::mk3(x[3], x[4], x[5]), x[6]); y[0] = r.x; y[1] = r.y; y[2] = r.z;)
// ---- the specified algorithms (AC5 and its kin) and AC6
DA_OP(sincos_ac, 1, 2, pt::sincos_ac(x[0], y[0], y[1]);)
DA_OP(exp_ac, 1, 1, y[0] = pt::exp_ac(x[0]);)
DA_OP(pow_int_ac, 2, 1, y[0] = pt::pow_int_ac(x[0], (int)pt::f2i(x[1]));)   // x[1]: the bits of n >= 1
DA_OP(atan2_ac, 2, 1, y[0] = pt::atan2_ac(x[0], x[1]);)
DA_OP(pow22, 1, 1, y[0] = pt::pow22(x[0]);)
DA_OP(disney_consts, 7, 6, pt::v3 a; pt::v3 b; pt::disney_color_constants(pt::mk3(x[0], x[1], x[2]), x[3], x[4], x[5], x[6], a, b);
      y[0] = a.x; y[1] = a.y; y[2] = a.z; y[3] = b.x; y[4] = b.y; y[5] = b.z;)
// ---- the node step's sort: x[0..3] entry distances, x[4..7] the bits of the child references; the 5-exchange network of node_step_nearfar
DA_OP(childkey, 8, 8,
      pt::ChildKey k[4];
      for (int c = 0; c < 4; c++) k[c] = pt::ChildKey::make(x[c], (int)pt::f2i(x[4 + c]));
      pt::ChildKey::order(k[0], k[1]); pt::ChildKey::order(k[2], k[3]); pt::ChildKey::order(k[0], k[2]);
      pt::ChildKey::order(k[1], k[3]); pt::ChildKey::order(k[1], k[2]);
      for (int c = 0; c < 4; c++) { y[c] = k[c].t(); y[4 + c] = pt::i2f((int32_t)k[c].ref()); })
// ---- device only: the hardware approximations behind fast_shading, the WINDOW prefilter and the packet kernel's node step
#if defined(DA_DEVICE_OP)
DA_DEVICE_OP(hw_rcp, 1, 1, y[0] = pt::ShadeMath<true>::rcp(x[0]);)
DA_DEVICE_OP(hw_sqrt, 1, 1, y[0] = pt::ShadeMath<true>::sqrt(x[0]);)
DA_DEVICE_OP(hw_rsq, 1, 1, y[0] = __builtin_amdgcn_rsqf(x[0]);)
DA_DEVICE_OP(node_inv, 1, 1, y[0] = pt::node_inv(x[0]);)
#endif
