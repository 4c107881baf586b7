// bote_capi.hpp — shared by the C ABI's translation units (bote_capi.hip: the
// planet handle, the per-call entries, the chain search; bote_capi_sweep.hip:
// the sweep handle; bote_capi_search.hip: the multi-device search handle).
// Internal, not installed: the last-error slot, the device buffer and device
// guard, and the two handles that more than one unit reads.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/bote_hip.h"
#include "bote_host.hpp"
#include "bote_kernels.hpp"
#include "bote_pinned.hpp"

namespace bote {
namespace capi __attribute__((visibility("hidden"))) {

// bote_last_error()'s text: one per thread for the whole library (bote_capi.hip)
extern thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                          \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) return fail(BOTE_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

// An argument check of bote_host.hpp: its code and text, when it refuses
#define ARG_TRY(expr)                                  \
  do {                                                 \
    const bote::host::Status _s = (expr);              \
    if (_s.code) return fail(_s.code, _s.msg);         \
  } while (0)

// RAII device buffer; reserve() grows it (grow-only, for cached workspaces)
struct DBuf {
  void* p = nullptr;
  size_t cap = 0;
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t bytes) {
    cap = bytes ? bytes : 16;
    return hipMalloc(&p, cap);
  }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    const size_t old = cap;  // grow geometrically: a slightly larger call does not reallocate again
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    return alloc(std::max(bytes, 2 * old));
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return (T*)p; }
};

// Restores the calling thread's current HIP device when an entry returns:
// the entries switch to their planet's device, and the library must not
// leave the caller (a Rust or PyTorch host on another device) switched.
struct DevGuard {
  int dev = -1;
  DevGuard() {
    if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  }
  ~DevGuard() {
    if (dev >= 0) (void)hipSetDevice(dev);
  }
  DevGuard(const DevGuard&) = delete;
  DevGuard& operator=(const DevGuard&) = delete;
};

inline int device_cus(int dev) {
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 256;
  return prop.multiProcessorCount;
}

inline size_t device_max_lds(int dev) {
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
    return 160 * 1024;
  return (size_t)std::max(v, 160 * 1024);
}

inline void fill_rank_params(EvalArgs& a, const bote_ranking_params* rp) {
  a.want_score = rp ? 1 : 0;
  if (rp) {
    a.p_fmean = rp->min_mean_fpaxos_improv;
    a.p_emean = rp->min_mean_epaxos_improv;
    a.p_fair = rp->min_fairness_fpaxos_improv;
    a.ft_metric = rp->ft_metric;
  }
}

// Per launch range [rb, re) of a sweep, a table of start ranks on the device
// (the group kernel's work chunks, or the seed sample's one-step chunks) with
// each start's FastArgs::wstate (4 u64).
struct Chunks {
  std::vector<uint64_t> host;   // kept alive: the async upload reads it
  std::vector<uint64_t> state;  // per chunk: FastArgs::wstate (4 u64)
  DBuf dev, sdev;
  uint32_t n = 0;
};

// The tables of the last ranges launched (a bench or a shard re-launches the
// same range), at most CAP of them.
struct RangeCache {
  static constexpr size_t CAP = 16;
  std::map<std::pair<uint64_t, uint64_t>, std::unique_ptr<Chunks>> tables;
  // The table of [rb, re), or null with room made for it: a full cache is
  // emptied once the streams that may still read its device tables, the last
  // launch's and then `st`, have drained.
  hipError_t lookup(uint64_t rb, uint64_t re, hipStream_t last_stream, hipStream_t st, const Chunks*& out) {
    out = nullptr;
    auto it = tables.find({rb, re});
    if (it != tables.end()) {
      out = it->second.get();
      return hipSuccess;
    }
    if (tables.size() < CAP) return hipSuccess;
    hipError_t e = last_stream ? hipStreamSynchronize(last_stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) tables.clear();
    return e;
  }
  const Chunks* insert(uint64_t rb, uint64_t re, std::unique_ptr<Chunks> c) {
    return tables.emplace(std::make_pair(rb, re), std::move(c)).first->second.get();
  }
};

}  // namespace capi
}  // namespace bote

// A planet resident on one device.  The per-call entry points (bote_eval,
// bote_leaderless, ...) run stream-ordered on the planet's own non-blocking
// stream with cached, grow-only device workspaces; calls on one handle are
// serialised by its mutex, calls on distinct handles are independent (no
// device-wide synchronisation anywhere).
struct bote_planet {
  static constexpr size_t NWS = 14;  // (bote_eval's: 4 inputs, 10 outputs)
  int device;
  uint32_t R;
  std::vector<uint16_t> lat;
  uint32_t* d_mat = nullptr;
  hipStream_t stream = nullptr;
  mutable std::mutex mu;
  mutable bote::capi::DBuf ws[NWS];  // handed out per call by bote_capi.hip's Workspace
};

struct bote_sweep {
  using DBuf = bote::capi::DBuf;
  // the kernel that runs a launch: the generic one (bote_eval.hpp: any
  // planet), or the fast (bote_sweep.hip) or group (bote_group.hip) kernel
  // with the generic one as the exact fixup of the configs they defer.
  // Decided by sweep_plan_fast; bote_sweep_is_fast reports its value.
  enum class Path { Generic = 0, Fast = 1, Group = 2 };
  const bote_planet* p = nullptr;
  // the planet's device, kept here: bote_sweep_destroy may run after the
  // planet is gone (a garbage collector finalises the two in any order) and
  // must not read through `p`
  int device = 0;
  uint32_t n = 0, ns = 0, nc = 0, n_obj = 0, K = 0;
  bote::EvalArgs args{};
  uint32_t grid = 0, bd = 0;
  size_t shm = 0;
  DBuf srv, cli, binom, top, tmp0, tmp1, result, counters;
  // overflow fallback of the fast path (generic kernel over the whole range,
  // run only when the deferred queue overflowed; chosen on the device)
  DBuf top_alt, counters_alt;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipEvent_t last0 = nullptr, last1 = nullptr;  // the last launch's kernel events (ev0/ev1 or a timing slot)
  // recorded after the last work enqueued on the sweep's buffers (a launch's
  // merge chain, a result copy): destroy waits on it, not on the device
  hipEvent_t done = nullptr;
  // per-launch kernel timing since the last bote_sweep_timing_reset
  std::vector<std::pair<hipEvent_t, hipEvent_t>> evpool;
  size_t ev_used = 0;
  bool launched = false;
  Path path = Path::Generic;
  bool def_obj = false;  // the default objective set, compiled into the group kernel
  int tail = 0;          // bote::FAST_*: a MAX, percentile or MDTM objective picks the fast kernel's variant (never the group kernel)
  bote::FastArgs fargs{};  // fast and group kernels
  uint32_t fgrid = 0;
  size_t fshm = 0;
  uint32_t xgrid = 0;  // generic fixup grid (deferred configs)
  DBuf cqt, rqt, queue, qcount, lowtab;
  DBuf dbg;  // BOTE_DEBUG builds: device-assert flag bits
  DBuf pstats;  // BOTE_PATHSTATS builds: 64 path counters (group kernel)
  // group kernel work chunks per launch range, plus the ticket counter (wctr)
  bote::capi::RangeCache chunks;
  // top-K seed: the sample launch's one-step chunks per launch range, its
  // per-chunk minima and the seed keys
  bote::capi::RangeCache samples;
  DBuf smin, tseed;
  DBuf kbound;  // group lists' K-th key bound (FastArgs::kbound)
  // host walks of the groups (bote_host.hpp): one walk serves the split and
  // the chunk tables of every sub-range it covers (bote_search_* shares one
  // walk across its shards' sweeps)
  mutable std::vector<std::shared_ptr<const bote::host::GroupWalk>> walks;
  DBuf wctr;
  // a pinned sweep (bote_sweep_create_pinned; pin_n == 0: none): the sorted
  // pinned positions and its rank space C(ns - pin_n, n - pin_n)
  bote::PinArgs pz{};
  uint64_t ptotal = 0;
  // a constrained sweep (bote_sweep_create_constrained; n_con == 0: none):
  // args and fargs then hold n_obj + n_con key entries, the constraints last,
  // and `con` is what the constrained kernel variants take beside them
  // (bounds by key entry; its counter is set per launch).  admitted: [0] the
  // fast kernel's and its fix-up's count, or the generic path's; [1] the
  // overflow fallback's
  uint32_t n_con = 0;
  bote::ConArgs con{};
  DBuf admitted;
  uint64_t last_rb = 0, last_re = 0;
  hipStream_t last_stream = nullptr;
  uint64_t result_bytes() const { return (uint64_t)n_obj * bote::KP * 16 + 16; }
};

namespace bote {
namespace capi __attribute__((visibility("hidden"))) {
// bote_capi_sweep.hip, also called by the search handle: the group kernel's
// work-chunk table of [rb, re), uploaded on `st` (null off the group kernel),
// and bote_host's unpack_result on a sweep's result block
int sweep_chunks(bote_sweep* s, uint64_t rb, uint64_t re, hipStream_t st, const Chunks** out);
void unpack_result(const bote_sweep* s, const std::vector<uint8_t>& blk, bote_topk_record* out, uint32_t* out_count,
                   uint64_t* out_valid, uint64_t* out_digest);
// bote_capi_sweep.hip: a launch's merge chain over raw device buffers (the
// sweep's own, or bote_test_merge's): `lists` lists of `src`, or on the device
// `alt_lists` of `alt` when sel && *sel > cap, into `result` (n_obj x KP
// records, then the chosen counter pair at record lstride); tmp0 / tmp1 hold
// ceil(max(lists, alt_lists) / 8) lists each (the merge tree's levels)
int merge_lists(const Rec* src, uint32_t lists, const Rec* alt, uint32_t alt_lists, uint64_t lstride,
                const unsigned long long* sel, uint64_t cap, const unsigned long long* kbound, Rec* tmp0, Rec* tmp1,
                void* result, uint32_t n_obj, uint32_t K, const unsigned long long* counters,
                const unsigned long long* counters_alt, hipStream_t st);
}  // namespace capi
}  // namespace bote
