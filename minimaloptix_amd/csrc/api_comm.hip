// api_comm.hip -- multi-GPU collectives: one process per GPU, RCCL over xGMI.  The tile split of a frame, the run-time
// binding of RCCL, the deadline of a collective, and the moptix_comm_* / *_tiles / moptix_reduce_frame entry points of include/moptix.h.
#include <hip/hip_runtime.h>
#include <chrono>
#include <thread>
// RCCL's types and prototypes: from its header where there is one, else the handful this file needs (the library is bound at
// run time by name, see load_rccl; a build box without the RCCL package -- or `make EXTRA=-DMOPTIX_NO_RCCL_HEADER` -- still
// builds the whole library, and moptix_comm_* answer MOPTIX_ERR_STATE where no librccl can be loaded).
#if !defined(MOPTIX_NO_RCCL_HEADER) && __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0, ncclUnhandledCudaError = 1, ncclSystemError = 2, ncclInternalError = 3, ncclInvalidArgument = 4, ncclInvalidUsage = 5, ncclRemoteError = 6, ncclInProgress = 7 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3, ncclInt64 = 4, ncclUint64 = 5, ncclFloat16 = 6, ncclFloat32 = 7, ncclFloat = 7, ncclFloat64 = 8 } ncclDataType_t;
typedef enum { ncclSum = 0, ncclProd = 1, ncclMax = 2, ncclMin = 3 } ncclRedOp_t;
ncclResult_t ncclGetUniqueId(ncclUniqueId* uniqueId);
ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId commId, int rank);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
const char* ncclGetErrorString(ncclResult_t result);
ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();
ncclResult_t ncclCommGetAsyncError(ncclComm_t comm, ncclResult_t* asyncError);
ncclResult_t ncclCommAbort(ncclComm_t comm);
}
#endif

#include <dlfcn.h>

#include <cstdlib>
#include <cstring>

#include "api_context.h"

using namespace pt;
using namespace pt::api;

namespace {

// ---- tile split: a rank's tiles <-> a dense buffer (work-item order of megakernel.h item_to_pixel) ----
struct TileDeal { int nItems, tilesX, rank, nRanks, width, height; };
__device__ __forceinline__ bool deal_pixel(const TileDeal& d, int i, int& pixel) {
  const int lt = i >> 6, in = i & 63;
  const int gt = lt * d.nRanks + (d.rank + lt) % d.nRanks;
  const int tx = gt % d.tilesX, ty = gt / d.tilesX;
  const int x = tx * 8 + (in & 7), y = ty * 8 + (in >> 3);
  pixel = y * d.width + x;
  return (x < d.width) & (y < d.height);
}
__global__ void __launch_bounds__(256) k_pack_tiles(const float* __restrict__ accum, float* __restrict__ packed, TileDeal d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.nItems) return;
  int px; float r = 0.f, g = 0.f, b = 0.f;
  if (deal_pixel(d, i, px)) { r = accum[3 * (size_t)px]; g = accum[3 * (size_t)px + 1]; b = accum[3 * (size_t)px + 2]; }
  packed[3 * (size_t)i] = r; packed[3 * (size_t)i + 1] = g; packed[3 * (size_t)i + 2] = b;
}
__global__ void __launch_bounds__(256) k_unpack_tiles(const float* __restrict__ packed, float* __restrict__ accum, TileDeal d) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= d.nItems) return;
  int px;
  if (deal_pixel(d, i, px)) { accum[3 * (size_t)px] = packed[3 * (size_t)i]; accum[3 * (size_t)px + 1] = packed[3 * (size_t)i + 1]; accum[3 * (size_t)px + 2] = packed[3 * (size_t)i + 2]; }
}
int tile_deal(moptix_context c, int rank, int nRanks, TileDeal& d) {
  if (!c->haveParams) return fail(c, MOPTIX_ERR_STATE, "no params");
  if (nRanks < 1 || rank < 0 || rank >= nRanks) return fail(c, MOPTIX_ERR_INVALID, "bad partition");
  const int tilesX = ((int)c->params.width + 7) / 8, tilesY = ((int)c->params.height + 7) / 8;
  const long long localTiles = ((long long)tilesX * tilesY + nRanks - 1) / nRanks;
  if (localTiles * 64 > 0x7fffffffLL) return fail(c, MOPTIX_ERR_LIMIT, "frame too large");
  d.nItems = (int)(localTiles * 64); d.tilesX = tilesX; d.rank = rank; d.nRanks = nRanks;
  d.width = (int)c->params.width; d.height = (int)c->params.height;
  return MOPTIX_OK;
}
// RCCL is bound at the first moptix_comm_* call, not at load time: a host process that already carries an RCCL (PyTorch
// ships its own librccl.so.1) must keep exactly one copy, and a process that never goes multi-GPU needs none.  dlopen by
// soname returns the copy that is already loaded, else the one on this library's run path (/opt/rocm/lib).
struct RcclApi {
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr; decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr; decltype(&ncclGetErrorString) GetErrorString = nullptr;
  decltype(&ncclSend) Send = nullptr; decltype(&ncclRecv) Recv = nullptr; decltype(&ncclReduce) Reduce = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr; decltype(&ncclGroupEnd) GroupEnd = nullptr;
  // optional (used by comm_wait when the library has them): error state of a communicator without blocking, and tearing one down
  // while its kernels are still on the stream
  decltype(&ncclCommGetAsyncError) CommGetAsyncError = nullptr; decltype(&ncclCommAbort) CommAbort = nullptr;
  // optional: a NON-BLOCKING communicator (config.blocking = 0).  With a blocking one ncclSend / ncclGroupEnd / ncclReduce may sit inside
  // the library while the links to a peer are set up -- a peer that is alive but never calls blocks the host there, where no deadline of
  // ours can reach.  A non-blocking communicator returns ncclInProgress instead and the state is polled (comm_settle)
  decltype(&ncclCommInitRankConfig) CommInitRankConfig = nullptr;
  bool ok = false; std::string error;
};
// MOPTIX_RCCL_LIB names another library with the same nine entry points (a transport plug point; tests/rccl_loopback is a
// loop-back transport that lets the N > 1 branches below run as N processes on a ONE-GPU box, where RCCL itself refuses a
// communicator whose ranks share a device).  Loaded once; the C++11 static makes the first call thread-safe.
RcclApi load_rccl() {
  RcclApi api;
  const char* override_ = getenv("MOPTIX_RCCL_LIB");
  void* h = nullptr;
  if (override_ && *override_) {
    h = dlopen(override_, RTLD_NOW | RTLD_LOCAL);
    if (!h) { api.error = std::string("cannot load MOPTIX_RCCL_LIB: ") + dlerror(); return api; }
  } else {
    h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { api.error = std::string("cannot load librccl: ") + dlerror(); return api; }
  }
  bool all = true;
  auto sym = [&](const char* n) { void* p = dlsym(h, n); if (!p) { all = false; api.error = std::string("librccl lacks ") + n; } return p; };
  api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId"); api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
  api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy"); api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
  api.Send = (decltype(api.Send))sym("ncclSend"); api.Recv = (decltype(api.Recv))sym("ncclRecv"); api.Reduce = (decltype(api.Reduce))sym("ncclReduce");
  api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart"); api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
  api.ok = all;
  api.CommGetAsyncError = (decltype(api.CommGetAsyncError))dlsym(h, "ncclCommGetAsyncError");
  api.CommAbort = (decltype(api.CommAbort))dlsym(h, "ncclCommAbort");
  api.CommInitRankConfig = (decltype(api.CommInitRankConfig))dlsym(h, "ncclCommInitRankConfig");
  return api;
}
RcclApi& rccl() {
  static RcclApi api = load_rccl();
  return api;
}
int ncclFail(moptix_context c, ncclResult_t r, const char* what) {
  return fail(c, MOPTIX_ERR_HIP, std::string(what) + ": " + rccl().GetErrorString(r));
}
#define RCCL_READY(c) do { if (!rccl().ok) return fail((c), MOPTIX_ERR_STATE, rccl().error); } while (0)
#define NCCLCHK(c, x, what) do { ncclResult_t r_ = (x); if (r_ != ncclSuccess) return ncclFail((c), r_, (what)); } while (0)

// The end of a collective: wait for the context's stream WITH A DEADLINE.  A collective's kernels spin on the device until every
// peer has joined; a peer that died or never calls leaves them spinning, and a bare hipStreamSynchronize would then block this
// rank for good (only the CLI's --spawn parent has its own deadline).  So the stream is polled; each poll asks the communicator
// for an asynchronous error (a peer's process gone, a link down); on an error or after "comm_timeout_ms" the communicator is
// ABORTED (ncclCommAbort makes its kernels leave), the stream is given a bounded time to drain, and the call returns
// MOPTIX_ERR_COMM: the host is expected to exit (bench.py, class MinimalOptiX and dist.py raise).  The context keeps working
// as a one-rank context; a new communicator needs moptix_comm_init again.
// Tears a communicator down whose kernels or host-side operations cannot complete.  With ncclCommAbort its kernels leave and its
// resources go; WITHOUT it the communicator is leaked -- ncclCommDestroy waits for outstanding work, i.e. for the very thing that
// does not come.  The stream gets a bounded time to drain; if it has not by then the context is marked unusable (every later call
// returns MOPTIX_ERR_COMM): kernels of a dead collective still sit on its stream.
int comm_teardown(moptix_context c, const char* what, const std::string& why) {
  using clock = std::chrono::steady_clock;
  bool leaked = false;
  if (c->comm.handle) {
    if (rccl().CommAbort) (void)rccl().CommAbort(c->comm.handle); else leaked = true;
    c->comm.handle = nullptr; c->comm.rank = 0; c->comm.ranks = 1; c->comm.nonBlocking = false;
  }
  const auto t1 = clock::now();                     // the aborted kernels leave; never wait for them without a bound either
  while (hipStreamQuery(c->stream) == hipErrorNotReady && clock::now() - t1 < std::chrono::seconds(10)) std::this_thread::sleep_for(std::chrono::milliseconds(1));
  const bool busy = hipStreamQuery(c->stream) == hipErrorNotReady;
  if (busy) c->poisoned = true;
  return fail(c, MOPTIX_ERR_COMM, std::string(what) + ": " + why + (leaked ? "; the communicator was abandoned (this library has no ncclCommAbort)" : "; the communicator was aborted") +
                                  (busy ? "; its kernels are still on the stream: this context is unusable from here on" : ""));
}
// After a call on a NON-BLOCKING communicator: ncclInProgress means the library is still working on it in the background (setting links
// up, waiting for the peer's side of a connection); nothing else may be issued on the communicator until that has settled.  Polled
// against the same deadline as the device side ("comm_timeout_ms"); a hard error or the deadline tears the communicator down.
int comm_settle(moptix_context c, ncclResult_t r, const char* what) {
  using clock = std::chrono::steady_clock;
  if (r == ncclSuccess) return MOPTIX_OK;
  if (r != ncclInProgress || !c->comm.nonBlocking || !c->comm.handle) return ncclFail(c, r, what);
  const auto t0 = clock::now();
  const auto deadline = std::chrono::milliseconds(c->opt.commTimeoutMs);
  for (unsigned spin = 0;; spin++) {
    ncclResult_t st = ncclSuccess;
    const ncclResult_t q = rccl().CommGetAsyncError(c->comm.handle, &st);
    if (q != ncclSuccess) return comm_teardown(c, what, std::string("ncclCommGetAsyncError: ") + rccl().GetErrorString(q));
    if (st == ncclSuccess) return MOPTIX_OK;
    if (st != ncclInProgress) return comm_teardown(c, what, std::string("communicator reports ") + rccl().GetErrorString(st));
    if (clock::now() - t0 > deadline)
      return comm_teardown(c, what, "still in progress on the host after comm_timeout_ms = " + std::to_string(c->opt.commTimeoutMs) + " (a peer is alive but has not made its call)");
    if (spin < 4096) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
}
int comm_wait(moptix_context c, const char* what) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  const auto deadline = std::chrono::milliseconds(c->opt.commTimeoutMs);
  std::string why;
  for (unsigned spin = 0;; spin++) {
    const hipError_t q = hipStreamQuery(c->stream);
    if (q == hipSuccess) return MOPTIX_OK;
    if (q != hipErrorNotReady) return hipFail(c, q, what);
    ncclResult_t aerr = ncclSuccess;
    if (c->comm.handle && rccl().CommGetAsyncError && rccl().CommGetAsyncError(c->comm.handle, &aerr) == ncclSuccess && aerr != ncclSuccess && aerr != ncclInProgress) {
      why = std::string("communicator reports ") + rccl().GetErrorString(aerr); break;
    }
    if (clock::now() - t0 > deadline) { why = "no completion within comm_timeout_ms = " + std::to_string(c->opt.commTimeoutMs) + " (a peer is missing or late)"; break; }
    if (spin < 4096) std::this_thread::yield(); else std::this_thread::sleep_for(std::chrono::microseconds(100));
  }
  return comm_teardown(c, what, why);
}

}  // namespace

namespace pt { namespace api {
void comm_release(moptix_context c) {
  c->comm.tileSend.release(); c->comm.tileRecv.release();
  if (c->comm.handle) { (void)rccl().CommDestroy(c->comm.handle); c->comm.handle = nullptr; }
}
}}  // namespace pt::api

extern "C" {

int moptix_comm_unique_id(uint8_t* id128) {
  if (!id128) return fail(nullptr, MOPTIX_ERR_INVALID, "null id");
  static_assert(sizeof(ncclUniqueId) == MOPTIX_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (!rccl().ok) return fail(nullptr, MOPTIX_ERR_STATE, rccl().error);
  ncclResult_t r = rccl().GetUniqueId(&id);
  if (r != ncclSuccess) return ncclFail(nullptr, r, "ncclGetUniqueId");
  memcpy(id128, &id, sizeof(id));
  return MOPTIX_OK;
}

int moptix_comm_init(moptix_context c, const uint8_t* id128, int32_t rank, int32_t nRanks) {
  if (!c || !id128 || nRanks < 1 || rank < 0 || rank >= nRanks) return fail(c, MOPTIX_ERR_INVALID, "bad communicator arguments");
  RCCL_READY(c);
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if (c->comm.handle) { (void)rccl().CommDestroy(c->comm.handle); c->comm.handle = nullptr; }
  ncclUniqueId id; memcpy(&id, id128, sizeof(id));
  c->comm.nonBlocking = false;
  // Non-blocking where the library can do it and can also be polled and aborted ("comm_blocking" = 1 forces the plain form): every later
  // call then returns at once, ncclInProgress while the library still works on it, and comm_settle polls that state against
  // "comm_timeout_ms" -- a peer that is alive but never calls can no longer hold this rank inside ncclGroupEnd / ncclSend for good.
  if (!c->opt.commBlocking && rccl().CommInitRankConfig && rccl().CommGetAsyncError && rccl().CommAbort) {
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    const ncclResult_t r = rccl().CommInitRankConfig(&c->comm.handle, nRanks, id, rank, &cfg);
    c->comm.nonBlocking = true; c->comm.rank = rank; c->comm.ranks = nRanks;
    const int rc = comm_settle(c, r, "ncclCommInitRankConfig");
    if (rc != MOPTIX_OK) { c->comm.nonBlocking = false; c->comm.rank = 0; c->comm.ranks = 1; return rc; }
    return MOPTIX_OK;
  }
  NCCLCHK(c, rccl().CommInitRank(&c->comm.handle, nRanks, id, rank), "ncclCommInitRank");
  c->comm.rank = rank; c->comm.ranks = nRanks;
  return MOPTIX_OK;
}

int moptix_comm_destroy(moptix_context c) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (c->comm.handle) { HIPCHK(c, hipSetDevice(c->device), "hipSetDevice"); (void)hipStreamSynchronize(c->stream); NCCLCHK(c, rccl().CommDestroy(c->comm.handle), "ncclCommDestroy"); c->comm.handle = nullptr; }
  c->comm.rank = 0; c->comm.ranks = 1;
  return MOPTIX_OK;
}

int moptix_packed_tile_floats(moptix_context c, int32_t nRanks, uint64_t* out) {
  if (!c || !out) return MOPTIX_ERR_INVALID;
  TileDeal d; int rc = tile_deal(c, 0, nRanks, d);
  if (rc != MOPTIX_OK) return rc;
  *out = 3ull * (uint64_t)d.nItems;
  return MOPTIX_OK;
}

int moptix_pack_tiles(moptix_context c, int32_t rank, int32_t nRanks, float* dstDevice) {
  if (!c || !dstDevice) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  TileDeal d; int rc = tile_deal(c, rank, nRanks, d);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if ((rc = ensure_accum(c)) != MOPTIX_OK) return rc;
  k_pack_tiles<<<dim3((d.nItems + 255) / 256), dim3(256), 0, c->stream>>>(accum_ptr(c), dstDevice, d);
  HIPCHK(c, hipGetLastError(), "pack tiles");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_unpack_tiles(moptix_context c, int32_t rank, int32_t nRanks, const float* srcDevice) {
  if (!c || !srcDevice) return fail(c, MOPTIX_ERR_INVALID, "null argument");
  TileDeal d; int rc = tile_deal(c, rank, nRanks, d);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if ((rc = ensure_accum(c)) != MOPTIX_OK) return rc;
  c->accumPlain = true;                                      // samples without per-pixel counts (api_adaptive.hip)
  k_unpack_tiles<<<dim3((d.nItems + 255) / 256), dim3(256), 0, c->stream>>>(srcDevice, accum_ptr(c), d);
  HIPCHK(c, hipGetLastError(), "unpack tiles");
  HIPCHK(c, hipStreamSynchronize(c->stream), "sync");
  return MOPTIX_OK;
}

int moptix_gather_tiles(moptix_context c, int32_t dstRank) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (!c->comm.handle) return fail(c, MOPTIX_ERR_STATE, "moptix_comm_init has not been called");
  if (c->nRanks != c->comm.ranks || c->rank != c->comm.rank) return fail(c, MOPTIX_ERR_STATE, "moptix_set_partition does not match the communicator's rank / size");
  if (dstRank < 0 || dstRank >= c->comm.ranks) return fail(c, MOPTIX_ERR_INVALID, "bad destination rank");
  int rc = moptix_sync(c);
  if (rc != MOPTIX_OK) return rc;
  TileDeal d;
  if ((rc = tile_deal(c, c->rank, c->nRanks, d)) != MOPTIX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if ((rc = ensure_accum(c)) != MOPTIX_OK) return rc;
  const size_t cnt = 3 * (size_t)d.nItems;                   // the same on every rank: whole groups of nRanks tiles
  const int n = c->comm.ranks;
  if (n == 1) return MOPTIX_OK;                              // the frame is already in place
  const dim3 grid((d.nItems + 255) / 256), block(256);
  if (c->rank != dstRank) {
    HIPCHK(c, c->comm.tileSend.ensure(cnt), "alloc tile staging");
    k_pack_tiles<<<grid, block, 0, c->stream>>>(accum_ptr(c), c->comm.tileSend.p, d);
    HIPCHK(c, hipGetLastError(), "pack tiles");
    if ((rc = comm_settle(c, rccl().Send(c->comm.tileSend.p, cnt, ncclFloat, dstRank, c->comm.handle, c->stream), "ncclSend")) != MOPTIX_OK) return rc;
  } else {
    HIPCHK(c, c->comm.tileRecv.ensure(cnt * (size_t)n), "alloc tile staging");
    NCCLCHK(c, rccl().GroupStart(), "ncclGroupStart");
    ncclResult_t recvErr = ncclSuccess;
    for (int r = 0; r < n && (recvErr == ncclSuccess || recvErr == ncclInProgress); r++)
      if (r != dstRank) recvErr = rccl().Recv(c->comm.tileRecv.p + cnt * (size_t)r, cnt, ncclFloat, r, c->comm.handle, c->stream);
    const ncclResult_t endErr = rccl().GroupEnd();           // always: a group left open would swallow every later call of this thread
    if (recvErr != ncclSuccess && recvErr != ncclInProgress) return ncclFail(c, recvErr, "ncclRecv");
    // the receives are on the stream only once the group has settled (non-blocking communicator): the unpack kernels go behind them
    if ((rc = comm_settle(c, endErr, "ncclGroupEnd")) != MOPTIX_OK) return rc;
    c->accumPlain = true;                                    // samples without per-pixel counts (api_adaptive.hip)
    for (int r = 0; r < n; r++) {                            // the other ranks' tiles into this rank's accuBuffer
      if (r == dstRank) continue;
      TileDeal dr = d; dr.rank = r;
      k_unpack_tiles<<<grid, block, 0, c->stream>>>(c->comm.tileRecv.p + cnt * (size_t)r, accum_ptr(c), dr);
    }
    HIPCHK(c, hipGetLastError(), "unpack tiles");
  }
  return comm_wait(c, "moptix_gather_tiles");
}

int moptix_reduce_frame(moptix_context c, int32_t dstRank) {
  if (!c) return MOPTIX_ERR_INVALID;
  if (!c->comm.handle) return fail(c, MOPTIX_ERR_STATE, "moptix_comm_init has not been called");
  if (dstRank < 0 || dstRank >= c->comm.ranks) return fail(c, MOPTIX_ERR_INVALID, "bad destination rank");
  int rc = moptix_sync(c);
  if (rc != MOPTIX_OK) return rc;
  HIPCHK(c, hipSetDevice(c->device), "hipSetDevice");
  if ((rc = ensure_accum(c)) != MOPTIX_OK) return rc;
  if (c->comm.ranks > 1) c->accumPlain = true;               // samples without per-pixel counts (api_adaptive.hip)
  if (c->comm.ranks > 1 && (rc = comm_settle(c, rccl().Reduce(accum_ptr(c), accum_ptr(c), 3 * c->accumPixels, ncclFloat, ncclSum, dstRank, c->comm.handle, c->stream), "ncclReduce")) != MOPTIX_OK)
    return rc;
  return c->comm.ranks > 1 ? comm_wait(c, "moptix_reduce_frame") : moptix_sync(c);
}

}  // extern "C"
