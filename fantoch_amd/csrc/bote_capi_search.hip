// bote_capi_search.hip — the multi-device search handle of the C ABI
// (include/bote_hip.h), over the sweep handle of bote_capi_sweep.hip.
// the whole sharded search without PyTorch.  A bote_search
// holds, per shard i of [rank_begin, rank_end), a sweep on planets[i]'s device
// with a stream of its own, its rank bounds (equal estimated cost: one host
// walk of the groups, shared by every shard's sweep) and its uploaded
// work-chunk table; plus the gather and merge buffers on planets[0]'s device.
// A launch is then device work only: every shard's sweep and merge chain, a
// peer copy of its result block to the root device, and a deterministic
// (key, rank) merge tree there.  The result equals one unsharded sweep (the
// merge order does not depend on the number of shards).  Reference: the only
// parallelism of the reference search is rayon over client sets
// (search.rs:209-231); this replaces it for one client set over a node's GPUs.
#include "bote_capi.hpp"

using namespace bote::host;
using namespace bote::capi;

struct bote_search {
  struct Shard {
    bote_sweep* sw = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t done = nullptr;
    DBuf local;  // the shard's result block on its own device (remote shards)
    uint64_t b = 0, e = 0;
    int dev = 0;
  };
  std::vector<Shard> sh;
  int root = 0;
  hipStream_t rst = nullptr;
  // recorded on rst after a launch's last merge: the next launch's shard
  // streams wait on it before they overwrite `gathered` (a launch may follow
  // a launch without a result() between them)
  hipEvent_t merged_ev = nullptr;
  DBuf gathered, bufa, bufb, merged;
  uint64_t nb = 0;
  uint64_t rb = 0, re = 0;
  bool launched = false;
};

namespace {
// Drains every stream of the handle, then frees it (any state, error paths too).
void search_free(bote_search* h) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!h) return;
  for (auto& x : h->sh) {
    if (x.st) {
      (void)hipSetDevice(x.dev);
      (void)hipStreamSynchronize(x.st);
    }
  }
  if (h->rst) {
    (void)hipSetDevice(h->root);
    (void)hipStreamSynchronize(h->rst);
    (void)hipStreamDestroy(h->rst);
  }
  if (h->merged_ev) {
    (void)hipSetDevice(h->root);
    (void)hipEventDestroy(h->merged_ev);
  }
  for (auto& x : h->sh) {
    (void)hipSetDevice(x.dev);
    if (x.done) (void)hipEventDestroy(x.done);
    if (x.st) (void)hipStreamDestroy(x.st);
    if (x.sw) bote_sweep_destroy(x.sw);
    x.local.release();
  }
  (void)hipSetDevice(h->root);
  delete h;
}

// hipError_t -> BOTE_E_DEVICE with context (no early return past cleanup)
int hip_fail(hipError_t e, const char* what) {
  return fail(BOTE_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
}  // namespace

extern "C" {

int bote_search_create(const bote_planet* const* planets, uint32_t n_devices, const uint32_t* servers, uint32_t ns,
                       const uint32_t* clients, uint32_t nc, uint32_t n, uint64_t rank_begin, uint64_t rank_end,
                       const bote_objective* objs, uint32_t n_obj, uint32_t K, const bote_ranking_params* rp,
                       int digest, uint32_t keys, bote_search** out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!out) return fail(BOTE_E_ARG, "out is null");
  *out = nullptr;
  if (!planets || n_devices == 0) return fail(BOTE_E_ARG, "no planets");
  if (n_devices > 1024) return fail(BOTE_E_RANGE, "at most 1024 shards");
  for (uint32_t i = 0; i < n_devices; ++i) {
    if (!planets[i]) return fail(BOTE_E_ARG, "planet is null");
    if (planets[i]->R != planets[0]->R || planets[i]->lat != planets[0]->lat)
      return fail(BOTE_E_ARG, "the shards' planets differ");
  }
  if (n > ns) return fail(BOTE_E_ARG, "config size larger than the server list");
  ARG_TRY(check_rank_span(ns, n, rank_begin, rank_end));
  auto* h = new bote_search();
  h->sh = std::vector<bote_search::Shard>(n_devices);
  h->root = planets[0]->device;
  h->rb = rank_begin;
  h->re = rank_end;
  auto cleanup = [&](int code) {
    search_free(h);
    return code;
  };
  hipError_t e;
  int rc;
  for (uint32_t i = 0; i < n_devices; ++i) {
    auto& x = h->sh[i];
    x.dev = planets[i]->device;
    if ((rc = bote_sweep_create_keys(planets[i], servers, ns, clients, nc, n, objs, n_obj, K, rp, digest,
                                     BOTE_KERNEL_AUTO, keys, &x.sw)))
      return cleanup(rc);
    if ((e = hipSetDevice(x.dev)) != hipSuccess) return cleanup(hip_fail(e, "hipSetDevice (shard)"));
    if ((e = hipStreamCreateWithFlags(&x.st, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&x.done, hipEventDisableTiming)) != hipSuccess)
      return cleanup(hip_fail(e, "shard stream/event"));
  }
  // shards of equal estimated cost from one walk of the groups, shared by
  // every shard's sweep (their chunk tables are cut from it)
  std::vector<uint64_t> bnd((size_t)n_devices + 1);
  if ((rc = bote_sweep_split(h->sh[0].sw, rank_begin, rank_end, n_devices, bnd.data()))) return cleanup(rc);
  for (uint32_t i = 1; i < n_devices; ++i)
    for (const auto& w : h->sh[0].sw->walks) h->sh[i].sw->walks.push_back(w);
  for (uint32_t i = 0; i < n_devices; ++i) {
    auto& x = h->sh[i];
    x.b = bnd[i];
    x.e = bnd[i + 1];
    const Chunks* ch = nullptr;
    if ((e = hipSetDevice(x.dev)) != hipSuccess) return cleanup(hip_fail(e, "hipSetDevice (shard)"));
    if ((rc = sweep_chunks(x.sw, x.b, x.e, x.st, &ch))) return cleanup(rc);
  }
  // gather + merge buffers on the root device
  h->nb = h->sh[0].sw->result_bytes();
  const size_t groups = (n_devices + bote::G_MERGE_LISTS - 1) / bote::G_MERGE_LISTS;
  if ((e = hipSetDevice(h->root)) != hipSuccess) return cleanup(hip_fail(e, "hipSetDevice (root)"));
  if ((e = hipStreamCreateWithFlags(&h->rst, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipEventCreateWithFlags(&h->merged_ev, hipEventDisableTiming)) != hipSuccess)
    return cleanup(hip_fail(e, "root stream/event"));
  if (h->gathered.alloc(h->nb * n_devices) != hipSuccess || h->bufa.alloc(h->nb * groups) != hipSuccess ||
      h->bufb.alloc(h->nb * groups) != hipSuccess || h->merged.alloc(h->nb) != hipSuccess)
    return cleanup(fail(BOTE_E_NOMEM, "gather buffers"));
  for (auto& x : h->sh) {
    if (x.dev == h->root) continue;
    if ((e = hipSetDevice(x.dev)) != hipSuccess) return cleanup(hip_fail(e, "hipSetDevice (shard)"));
    if (x.local.alloc(h->nb) != hipSuccess) return cleanup(fail(BOTE_E_NOMEM, "shard result block"));
    // the shard's device writes its block into the root's memory: enable its
    // peer access to the root (xGMI), "already enabled" (another handle, or
    // the caller) counting as success; without peer access the copy is still
    // correct, staged through the host by the runtime
    int can = 0;
    if ((e = hipDeviceCanAccessPeer(&can, x.dev, h->root)) != hipSuccess)
      return cleanup(hip_fail(e, "hipDeviceCanAccessPeer"));
    if (can) {
      e = hipDeviceEnablePeerAccess(h->root, 0);
      if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();  // (clear the sticky "already enabled")
        e = hipSuccess;
      }
      if (e != hipSuccess) return cleanup(hip_fail(e, "hipDeviceEnablePeerAccess (shard to root)"));
    }
  }
  // the chunk uploads are stream-ordered before the first launch; drain them
  // here so that create returns with the handle idle
  for (auto& x : h->sh) {
    (void)hipSetDevice(x.dev);
    if ((e = hipStreamSynchronize(x.st)) != hipSuccess) return cleanup(hip_fail(e, "shard setup"));
  }
  (void)hipSetDevice(h->root);
  *out = h;
  return BOTE_OK;
}

int bote_search_bounds(const bote_search* h, uint64_t* out_bounds) {
  if (!h || !out_bounds) return fail(BOTE_E_ARG, "null argument");
  for (size_t i = 0; i < h->sh.size(); ++i) out_bounds[i] = h->sh[i].b;
  out_bounds[h->sh.size()] = h->sh.empty() ? h->rb : h->sh.back().e;
  return BOTE_OK;
}

int bote_search_launch(bote_search* h) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!h) return fail(BOTE_E_ARG, "search is null");
  int rc;
  hipError_t e;
  const uint32_t nd = (uint32_t)h->sh.size();
  // every shard first (asynchronous, one stream each: no host work between)
  for (auto& x : h->sh)
    if ((rc = bote_sweep_launch(x.sw, x.b, x.e, x.st))) return rc;
  for (uint32_t i = 0; i < nd; ++i) {
    auto& x = h->sh[i];
    char* dst = h->gathered.as<char>() + h->nb * i;
    // (write-after-read: the previous launch's merge tree may still be reading `gathered`)
    if (h->launched) {
      if ((e = hipSetDevice(x.dev)) != hipSuccess || (e = hipStreamWaitEvent(x.st, h->merged_ev, 0)) != hipSuccess)
        return hip_fail(e, "wait for the previous merge");
    }
    if (x.dev == h->root) {
      if ((rc = bote_sweep_result_device(x.sw, dst, x.st))) return rc;
    } else {
      if ((rc = bote_sweep_result_device(x.sw, x.local.p, x.st))) return rc;
      if ((e = hipMemcpyPeerAsync(dst, h->root, x.local.p, x.dev, h->nb, x.st)) != hipSuccess)
        return hip_fail(e, "peer copy of a shard result");
    }
    if ((e = hipSetDevice(x.dev)) != hipSuccess || (e = hipEventRecord(x.done, x.st)) != hipSuccess)
      return hip_fail(e, "record shard event");
  }
  if ((e = hipSetDevice(h->root)) != hipSuccess) return hip_fail(e, "hipSetDevice (root)");
  for (auto& x : h->sh)
    if ((e = hipStreamWaitEvent(h->rst, x.done, 0)) != hipSuccess) return hip_fail(e, "wait shard");
  // merge tree, at most 8 blocks per merge
  const char* src = h->gathered.as<char>();
  uint32_t m = nd;
  char* bufs[2] = {h->bufa.as<char>(), h->bufb.as<char>()};
  int bsel = 0;
  const bote_sweep* s0 = h->sh[0].sw;
  while (m > (uint32_t)bote::G_MERGE_LISTS) {
    const uint32_t groups = (m + bote::G_MERGE_LISTS - 1) / bote::G_MERGE_LISTS;
    for (uint32_t g = 0; g < groups; ++g) {
      const uint32_t k = std::min<uint32_t>(bote::G_MERGE_LISTS, m - bote::G_MERGE_LISTS * g);
      if ((rc = bote_merge_device(s0, src + (size_t)h->nb * bote::G_MERGE_LISTS * g, k, bufs[bsel] + (size_t)h->nb * g,
                                  h->rst)))
        return rc;
    }
    src = bufs[bsel];
    bsel ^= 1;
    m = groups;
  }
  if ((rc = bote_merge_device(s0, src, m, h->merged.p, h->rst))) return rc;
  if ((e = hipEventRecord(h->merged_ev, h->rst)) != hipSuccess) return hip_fail(e, "record merge event");
  h->launched = true;
  return BOTE_OK;
}

int bote_search_result(bote_search* h, bote_topk_record* out, uint32_t* out_count, uint64_t* out_valid,
                       uint64_t* out_digest) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!h) return fail(BOTE_E_ARG, "search is null");
  if (!h->launched) return fail(BOTE_E_ARG, "search not launched");
  HIP_TRY(hipSetDevice(h->root));
  std::vector<uint8_t> blk(h->nb);
  HIP_TRY(hipMemcpyAsync(blk.data(), h->merged.p, h->nb, hipMemcpyDeviceToHost, h->rst));
  HIP_TRY(hipStreamSynchronize(h->rst));
  unpack_result(h->sh[0].sw, blk, out, out_count, out_valid, out_digest);
  return BOTE_OK;
}

int bote_search_destroy(bote_search* h) {
  search_free(h);
  return BOTE_OK;
}

int bote_search_topk(const bote_planet* const* planets, uint32_t n_devices, const uint32_t* servers, uint32_t ns,
                     const uint32_t* clients, uint32_t nc, uint32_t n, uint64_t rank_begin, uint64_t rank_end,
                     const bote_objective* objs, uint32_t n_obj, uint32_t K, const bote_ranking_params* rp,
                     int digest, bote_topk_record* out, uint32_t* out_count, uint64_t* out_valid,
                     uint64_t* out_digest) {
  bote_search* h = nullptr;
  int rc = bote_search_create(planets, n_devices, servers, ns, clients, nc, n, rank_begin, rank_end, objs, n_obj, K,
                              rp, digest, BOTE_KEYS_BASE, &h);
  if (rc) return rc;
  if (!(rc = bote_search_launch(h))) rc = bote_search_result(h, out, out_count, out_valid, out_digest);
  const std::string err = g_err;
  search_free(h);
  if (rc) g_err = err;
  return rc;
}

}  // extern "C"
