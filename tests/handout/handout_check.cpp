// handout_check.cpp -- host check of the lean packet kernel's hand-out (csrc/megakernel.h handout_lean, magic_div) against the plain
// functions every other kernel keeps (handout_to_item -> item_to_pixel -> begin_sample's x, y).  Built and run by tests/test_handout_cpu.py:
//   handout_check small | large | magic
// Prints one summary line and exits 0, or the first mismatch and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "megakernel.h"

using namespace pt;

namespace {

long long g_checks = 0;

struct Case { int width, height, nSeeds, nRanks, rank, tileMajor; bool ordered; };

bool fail(const Case& c, int k, const char* what, long long oldV, long long newV) {
  printf("MISMATCH %s: old %lld new %lld at k=%d frame %dx%d nSeeds=%d rank %d/%d tile_major=%d order=%d\n", what, oldV, newV, k, c.width, c.height,
         c.nSeeds, c.rank, c.nRanks, c.tileMajor, (int)c.ordered);
  return false;
}

// one k: the mapping as the general kernels compute it against handout_lean
bool check_k(const Case& c, const LaunchArgs& a, const HandoutConsts& hc, int k) {
  const int item = handout_to_item(a, k);
  int sample, pixel;
  const bool in = item_to_pixel(a, item, sample, pixel);
  const int x = pixel % a.scene.width, y = pixel / a.scene.width;      // begin_sample
  WorkItem w;
  const bool inNew = handout_lean(a, &hc, k, w);
  g_checks++;
  if (in != inNew) return fail(c, k, "in-frame flag", in, inNew);
  if (item != w.item) return fail(c, k, "item", item, w.item);
  if (sample != w.sample) return fail(c, k, "sample", sample, w.sample);
  if (pixel != w.pixel) return fail(c, k, "pixel", pixel, w.pixel);
  if (in && (x != w.x || y != w.y)) return fail(c, k, x != w.x ? "x" : "y", x != w.x ? x : y, x != w.x ? w.x : w.y);
  return true;
}

// plan_launch's numbers for a frame and a partition
void plan(const Case& c, LaunchArgs& a, std::vector<int>& order, std::mt19937& rng) {
  memset(&a, 0, sizeof(a));
  a.scene.width = c.width; a.scene.height = c.height;
  const int tilesX = (c.width + 7) / 8, tilesY = (c.height + 7) / 8;
  const long long nTiles = (long long)tilesX * tilesY, localTiles = (nTiles + c.nRanks - 1) / c.nRanks;
  a.nItems = (int)(localTiles * 64); a.tilesX = tilesX; a.rank = c.rank; a.nRanks = c.nRanks;
  a.nSeeds = c.nSeeds; a.nWork = c.nSeeds * a.nItems;
  a.tileMajor = c.tileMajor; a.unitShift = c.tileMajor == 3 ? 0 : 6;
  order.clear();
  if (c.ordered && c.tileMajor) {      // a shuffled list of the rank's units: tiles, or pixel slots under tile_major 3
    order.resize((size_t)a.nItems >> a.unitShift);
    for (size_t i = 0; i < order.size(); i++) order[i] = (int)i;
    for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[rng() % i]);
    a.tileOrder = order.data();
  }
}

template <class EachK>
bool for_cases(const int (*frames)[2], int nFrames, EachK each) {
  static const int seeds[] = { 1, 3, 16, 255, 256 }, ranks[] = { 1, 2, 3, 8 };
  std::mt19937 rng(20260u);
  std::vector<int> order;
  for (int f = 0; f < nFrames; f++)
    for (int nSeeds : seeds) for (int nRanks : ranks) for (int rank = 0; rank < nRanks; rank++)
      for (int tm = 0; tm <= 3; tm++) for (int ordered = 0; ordered <= 1; ordered++) {
        const Case c = { frames[f][0], frames[f][1], nSeeds, nRanks, rank, tm, ordered != 0 };
        LaunchArgs a;
        plan(c, a, order, rng);
        const HandoutConsts hc = handout_consts(a.tileMajor, a.nItems, a.nSeeds, a.tilesX, a.nRanks);
        if (!each(c, a, hc)) return false;
      }
  return true;
}

bool run_small() {
  static const int frames[][2] = { { 8, 8 }, { 37, 19 } };
  return for_cases(frames, 2, [](const Case& c, const LaunchArgs& a, const HandoutConsts& hc) {
    for (int k = 0; k < a.nWork; k++) if (!check_k(c, a, hc, k)) return false;
    return true;
  });
}

bool run_large() {
  static const int frames[][2] = { { 1920, 1080 } };
  return for_cases(frames, 1, [](const Case& c, const LaunchArgs& a, const HandoutConsts& hc) {
    const int n = a.nWork, per = a.nSeeds << 6;
    for (int k = 0; k < 4096 && k < n; k++) if (!check_k(c, a, hc, k)) return false;
    for (int k = n > 4096 ? n - 4096 : 0; k < n; k++) if (!check_k(c, a, hc, k)) return false;
    for (int step : { per, a.nItems })
      for (long long m = 0; m <= n; m += step)
        for (long long k = m - 1; k <= m + 1; k++) if (k >= 0 && k < n && !check_k(c, a, hc, (int)k)) return false;
    return true;
  });
}

bool check_div(int d, long long n) {
  if (n < 0 || n > 0x7fffffffLL) return true;
  const MagicDiv m = magic_div(d);
  const int q = magic_quot((int)n, m), r = (int)n - q * d;
  g_checks++;
  if (q != (int)n / d || r != (int)n % d) { printf("MISMATCH %lld / %d: operators %d rem %d, multiply-and-shift %d rem %d (mul %u shift %u)\n", n, d, (int)n / d, (int)n % d, q, r, m.mul, m.shift); return false; }
  return true;
}

bool run_magic() {
  std::vector<int> ds = { 1, 2, 3, 5, 7, 64, 192, 240, 16320, 16384, (1 << 30) - 1, 0x7fffffff };
  std::mt19937_64 rng(20261u);
  for (int i = 0; i < 500; i++) ds.push_back(1 + (int)(rng() % 0x7fffffffull));                        // uniform: mostly large divisors
  for (int i = 0; i < 500; i++) { const int bits = 1 + (int)(rng() % 31); ds.push_back(1 + (int)(rng() % ((1ull << bits) - 1ull))); }      // every size: 1 .. 2^bits - 1
  for (int d : ds) {
    for (long long n : { 0LL, 1LL, (long long)d - 1, (long long)d, (long long)d + 1, 0x7fffffffLL }) if (!check_div(d, n)) return false;
    const long long multiples = 0x7fffffffLL / d;
    if (multiples <= (1LL << 20)) {
      for (long long j = 0; j <= multiples; j++) for (long long n = j * d - 1; n <= j * d + 1; n++) if (!check_div(d, n)) return false;
    } else {
      for (int i = 0; i < (1 << 20); i++) { const long long j = (long long)(rng() % (unsigned long long)(multiples + 1)); for (long long n = j * d - 1; n <= j * d + 1; n++) if (!check_div(d, n)) return false; }
    }
  }
  return true;
}

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  bool ok;
  if (!strcmp(mode, "small")) ok = run_small();
  else if (!strcmp(mode, "large")) ok = run_large();
  else if (!strcmp(mode, "magic")) ok = run_magic();
  else { fprintf(stderr, "usage: handout_check small | large | magic\n"); return 2; }
  if (!ok) return 1;
  printf("ok %s: %lld checks\n", mode, g_checks);
  return 0;
}
