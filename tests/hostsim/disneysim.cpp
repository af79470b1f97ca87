// disneysim.cpp -- TEST INFRASTRUCTURE.  The three Disney functions of minimaloptix_amd/csrc/pt_disney.h, called one at a time on the host:
// a moptix_material goes through make_dev_material (pt_upload.h), as moptix_add_material and hostsim_create put it through, and
// disney_sample / disney_pdf / the one-evaluation disney_eval run on arrays of directions or RNG states.  tests/test_material_cases_cpu.py
// compares the results with the oracle's orc_disney_* and with a binary64 restatement.  It is not part of the product: nothing under
// minimaloptix_amd/ builds or loads it.
#include "hostsim.h"
#include "../../minimaloptix_amd/csrc/pt_disney.h"

using namespace hostsim;

namespace {
inline v3 ld(const float* p, int64_t i) { return mk3(p[3 * i], p[3 * i + 1], p[3 * i + 2]); }
inline void st(float* p, int64_t i, v3 a) { p[3 * i] = a.x; p[3 * i + 1] = a.y; p[3 * i + 2] = a.z; }
}  // namespace

extern "C" {

// Per element i: the state states[i] draws disney_sample's three numbers; L, H (3 floats each) and the state afterwards come back.
int disneysim_sample(const moptix_material* m, int64_t n, const float* N, const float* V, uint32_t* states, float* L, float* H) {
  if (!m || n < 0 || (n > 0 && (!N || !V || !states || !L || !H))) return -1;
  const DevMaterial dm = make_dev_material(*m);
  for (int64_t i = 0; i < n; i++) {
    v3 l, h;
    disney_sample(states[i], dm, make_onb(ld(N, i)), ld(V, i), l, h);
    st(L, i, l); st(H, i, h);
  }
  return 0;
}

int disneysim_pdf(const moptix_material* m, int64_t n, const float* N, const float* L, const float* H, float* pdf) {
  if (!m || n < 0 || (n > 0 && (!N || !L || !H || !pdf))) return -1;
  const DevMaterial dm = make_dev_material(*m);
  for (int64_t i = 0; i < n; i++) pdf[i] = disney_pdf<false>(dm, ld(N, i), ld(L, i), ld(H, i));
  return 0;
}

// The untextured evaluation: the colour constants are the material record's own.
int disneysim_eval(const moptix_material* m, int64_t n, const float* N, const float* V, const float* L, const float* H, float* out) {
  if (!m || n < 0 || (n > 0 && (!N || !V || !L || !H || !out))) return -1;
  const DevMaterial dm = make_dev_material(*m);
  for (int64_t i = 0; i < n; i++)
    st(out, i, disney_eval<false>(dm, dm.Cdlin, dm.Cspec0, dm.Csheen, make_onb(ld(N, i)), ld(L, i), ld(V, i), ld(H, i)));
  return 0;
}

}  // extern "C"
