// api_options.hip -- moptix_set_option / moptix_get_option of include/moptix.h: one table serves both.
#include <climits>
#include <cstring>

#include "api_context.h"

using namespace pt;
using namespace pt::api;

namespace {

enum Invalidates { kNothing, kAccelIfChanged, kNodeFormat, kTileHistory, kFaceSnapshot };
// A row with a member is stored: it can be set and read.  A row with `read` is computed from the context and can only be read; a row with
// neither is an action, it can only be set.  Whatever a row cannot do answers "unknown option", as a name the table does not hold.
struct Option {
  const char* name;
  int Options::* member;
  int (*read)(moptix_context) = nullptr;
  int lo = 0, hi = 0;                 // accepted: lo..hi, or, with nValues > 0, exactly values[]
  const char* accepted = "";          // the same in words, for the error message: "NAME in [0,64]"
  Invalidates invalidates = kNothing;
  int nValues = 0, values[4] = { 0, 0, 0, 0 };
  bool can_set() const { return !read; }
  bool can_get() const { return member || read; }
};

static_assert(kMaxLeaf == 8, "leaf_size's message says [1,8]");
const Option kOptions[] = {
  { "exit_threshold", &Options::exitThreshold, nullptr, 0, 64, "in [0,64]" },
  { "leaf_size", &Options::leafSize, nullptr, 1, kMaxLeaf, "in [1,8]", kAccelIfChanged },
  { "blocks_per_cu", &Options::blocksPerCU, nullptr, 1, 8, "in [1,8]" },
  // -1: back to the library's own choice per launch (plan_launch: the packet kernel for long launches of eligible scenes)
  { "kernel_variant", &Options::kernelVariant, nullptr, 0, 0, "in {-1,0,3,4} (1 and 2 were removed in round 3)", kNothing, 4, { -1, 0, 3, 4 } },
  { "sample_buffer_mb", &Options::sampleBufMB, nullptr, 1, INT_MAX, ">= 1" },
  { "leaf_threshold", &Options::leafThreshold, nullptr, 1, 64, "in [1,64]" },
  { "swap_lanes", &Options::swapLanes, nullptr, 1, 64, "in [1,64]" },
  { "starve_lanes", &Options::starveLanes, nullptr, 1, 64, "in [1,64]" },
  { "tile_major", &Options::tileMajor, nullptr, 0, 3, "in {0,1,2,3}" },
  { "auto_packet", &Options::autoPacket, nullptr, 0, 1, "in {0,1}" },
  { "analytic_queue", &Options::analyticQueue, nullptr, -1, 1, "in {-1,0,1}" },
  { "aux_depth", &Options::auxDepth, nullptr, 0, 100000, "in [0,100000]" },
  { "drain_below", &Options::drainBelow, nullptr, 0, 64, "in [0,64]" },
  { "specialize", &Options::specialize, nullptr, 0, 1, "in {0,1}" },
  { "slots_in_use", &Options::slotsInUse, nullptr, -1, 1024, "in [-1,1024]" },
  { "builder", &Options::builder, nullptr, 0, 1, "in {0,1}", kAccelIfChanged },
  { "fast_shading", &Options::fastShading, nullptr, 0, 1, "in {0,1}" },
  { "node_format", &Options::nodeFormat, nullptr, 0, 0, "in {0,64,128}", kNodeFormat, 3, { 0, 64, 128 } },      // setting it, even to the same value, asks the scene again
  { "shadow_rule", &Options::shadowRule, nullptr, 0, 1, "in {0,1}" },
  { "watchdog_ms", &Options::watchdogMs, nullptr, 1, INT_MAX, ">= 1" },
  { "comm_timeout_ms", &Options::commTimeoutMs, nullptr, 1, INT_MAX, ">= 1" },
  { "comm_blocking", &Options::commBlocking, nullptr, 0, 1, "in {0,1}" },
  { "query_blocks_per_cu", &Options::queryBlocksPerCU, nullptr, 1, 64, "in [1,64]" },
  { "radiance_buffer_mb", &Options::radianceBufferMB, nullptr, 1, 16384, "in [1,16384]" },
  { "temporal_face_motion", &Options::temporalFaceMotion, nullptr, 0, 1, "in {0,1}", kFaceSnapshot },      // 0 drops the face snapshot
  { "forget_history", nullptr, nullptr, INT_MIN, INT_MAX, "", kTileHistory },      // the next launch orders its work like a context's first (measurement of a cold frame)
  { "comm_nonblocking_used", nullptr, [](moptix_context c) { return c->comm.nonBlocking ? 1 : 0; } },
  { "node_format_used", nullptr, [](moptix_context c) { return c->nodeFormatUsed; } },
  { "kernel_variant_used", nullptr, [](moptix_context c) { return c->lastVariant; } },
  { "kernel_features_used", nullptr, [](moptix_context c) { return c->lastFeatures; } },      // FEAT_* mask (pt_types.h) of the last render's trace kernel; 15 = every program
  { "kernel_slim_used", nullptr, [](moptix_context c) { return c->lastSlim; } },              // 1: that kernel was the packet kernel's slim build (packetkernel.hip)
  { "counted_span_us", nullptr, [](moptix_context c) { return c->countedSpanUs; } },
  { "counted_tail_us", nullptr, [](moptix_context c) { return c->countedTailUs; } },
  { "path_slots", nullptr, [](moptix_context) { return packetkernel_slots(); } },
  { "comm_ranks", nullptr, [](moptix_context c) { return c->comm.handle ? c->comm.ranks : 0; } },
  { "num_cus", nullptr, [](moptix_context c) { return c->numCUs; } },
};
const Option* find_option(const char* name) {
  for (const Option& o : kOptions) if (!strcmp(name, o.name)) return &o;
  return nullptr;
}

}  // namespace

extern "C" {

int moptix_set_option(moptix_context c, const char* name, int32_t value) {
  if (!c || !name) return MOPTIX_ERR_INVALID;
  const Option* o = find_option(name);
  if (!o || !o->can_set()) return fail(c, MOPTIX_ERR_INVALID, std::string("unknown option: ") + name);
  bool ok = o->nValues == 0 && value >= o->lo && value <= o->hi;
  for (int i = 0; i < o->nValues; i++) ok = ok || value == o->values[i];
  if (!ok) return fail(c, MOPTIX_ERR_INVALID, std::string(name) + " " + o->accepted);
  if (o->invalidates == kAccelIfChanged && value != c->opt.*o->member) c->accelBuilt = false;
  if (o->invalidates == kNodeFormat) c->formatDecided = false;
  if (o->invalidates == kTileHistory) c->tiles.forget();
  if (o->invalidates == kFaceSnapshot && value == 0 && c->tp.faces.prev.p) {      // the snapshot and its records go with the option
    (void)hipSetDevice(c->device);
    if (!c->poisoned) (void)hipStreamSynchronize(c->stream);
    c->tp.faces.release();
  }
  if (o->invalidates == kFaceSnapshot && value == 0) c->tp.faces.have = false;
  if (o->member) c->opt.*o->member = value;
  return MOPTIX_OK;
}

int moptix_get_option(moptix_context c, const char* name, int32_t* value) {
  if (!c || !name || !value) return MOPTIX_ERR_INVALID;
  const Option* o = find_option(name);
  if (!o || !o->can_get()) return fail(c, MOPTIX_ERR_INVALID, std::string("unknown option: ") + name);
  *value = o->member ? c->opt.*o->member : o->read(c);
  return MOPTIX_OK;
}

}  // extern "C"
