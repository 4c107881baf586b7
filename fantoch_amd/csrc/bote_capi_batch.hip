// bote_capi_batch.hip — the batch handle of the C ABI (include/bote_hip.h,
// bote_batch_*): many pinned sets of one size swept by one launch (DESIGN.md §4
// "Batched pinned sweeps").  Host work only (bote_capi.hip's header).
//
// A batch owns two pinned sweeps of its first set (bote_capi_sweep.hip), built
// by the public entry so that planning, refusals and uploads are the pinned
// sweep's own:
//   fast  on the fast path (null when the batch runs the generic kernel): its
//         planet layouts, fast-kernel arguments, LDS size and deferred queue
//         serve the batch kernel; the handle itself is never launched;
//   gen   on the generic kernel: launched once per set, with that set's
//         positions, on the generic path and for the recompute of a batch that
//         deferred configs.
// What the batch adds is the set table, the per-set list slots and counters
// and the B result blocks.  A bounded batch (bote_batch_create_bounded, DESIGN.md
// §4 "Streaming evolving search") also fills each set's two limits
// (PinArgs::lim): they travel in the set table to the batch kernel and, by
// value, with every per-set launch of `gen`.
#include "bote_capi.hpp"

using bote::EvalArgs;
using bote::Rec;
using Path = bote_sweep::Path;

using namespace bote::host;
using namespace bote::capi;

struct bote_batch {
  using DBuf = bote::capi::DBuf;
  int device = 0;
  uint32_t n = 0, ns = 0, n_obj = 0, K = 0, n_sets = 0, m = 0;
  bote_sweep* fast = nullptr;
  bote_sweep* gen = nullptr;
  std::vector<bote::PinArgs> sets;  // positions ascending
  BatchPlan plan;
  uint32_t grid = 0;
  // fast path: the set table, [n_sets][BATCH_SET_LISTS] list slots (unit lists,
  // all-ones padding), [n_sets][2] counters
  DBuf dsets, top, counters;
  DBuf result;  // [n_sets] result blocks (bote_sweep_result_device's layout)
  hipEvent_t e0 = nullptr, e1 = nullptr, done = nullptr;
  bool launched = false, recomputed = false;
  uint64_t block_bytes() const { return (uint64_t)n_obj * bote::KP * 16 + 16; }
};

namespace {

// every set on the generic kernel's pinned variant, each into its result block
int launch_per_set(bote_batch* b, hipStream_t st) {
  int rc;
  if ((rc = bote_sweep_timing_reset(b->gen))) return rc;
  for (uint32_t i = 0; i < b->n_sets; ++i) {
    b->gen->pz = b->sets[i];  // (the launch takes it by value)
    if ((rc = bote_sweep_launch(b->gen, 0, b->plan.total, st))) return rc;
    if ((rc = bote_sweep_result_device(b->gen, (char*)b->result.p + (size_t)i * b->block_bytes(), st))) return rc;
  }
  return BOTE_OK;
}

int launch_batch_fast(bote_batch* b, hipStream_t st) {
  const bote_sweep* s = b->fast;
  const uint64_t lstride = (uint64_t)b->n_obj * bote::KP;
  HIP_TRY(hipMemsetAsync(b->counters.p, 0, (size_t)b->n_sets * 16, st));
  HIP_TRY(hipMemsetAsync(s->qcount.p, 0, 8, st));
  bote::FastArgs f = s->fargs;
  f.out_top = b->n_obj ? b->top.as<Rec>() : nullptr;
  f.out_counters = b->counters.as<unsigned long long>();
  bote::BatchArgs z{};
  z.sets = b->dsets.as<bote::PinArgs>();
  z.n_sets = b->n_sets;
  z.slices = b->plan.slices;
  z.slice_len = b->plan.slice_len;
  z.ptotal = b->plan.total;
  z.runlen = b->plan.runlen;
  HIP_TRY(bote::launch_fast_batch(f, b->n, z, b->grid, s->fshm, st, b->e0, b->e1));
  // one merge level: a set's slots are one 8-way group, its output the set's result block
  if (b->n_obj)
    HIP_TRY(bote::launch_merge(b->top.as<Rec>(), b->n_sets * bote::BATCH_SET_LISTS, nullptr, 0, lstride, nullptr, 0,
                               b->result.as<Rec>(), lstride + 1, b->n_obj, st));
  HIP_TRY(hipMemcpy2DAsync((char*)b->result.p + lstride * 16, b->block_bytes(), b->counters.p, 16, 16, b->n_sets,
                           hipMemcpyDeviceToDevice, st));
  return BOTE_OK;
}

// bote_batch_create and, with `bounded`, bote_batch_create_bounded: prev_s1
// holds each set's previous-level Atlas sums, turned into the set's limits
// (PinArgs::lim) with rp's min_mean_decrease and ft_metric
int batch_create(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                 uint32_t n, const uint32_t* pinned, uint32_t n_sets, uint32_t n_pinned, uint32_t max_blocks,
                 const bote_objective* objs, uint32_t n_obj, uint32_t K, const bote_ranking_params* rp, int digest,
                 int kernel, bool bounded, const uint64_t* prev_s1, bote_batch** out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  bool has_score = false;
  if (!out) return fail(BOTE_E_ARG, "out is null");
  ARG_TRY(check_sweep_args(p ? p->R : 0, servers, ns, clients, nc, n, objs, n_obj, K, rp, kernel, 0, has_score));
  ARG_TRY(check_batch_args(ns, n, pinned, n_sets, n_pinned, 0));
  ARG_TRY(check_pinned_args(ns, n, pinned, n_pinned, kernel, 0));  // (a forced group kernel)
  if (bounded) ARG_TRY(check_bounded_args(prev_s1, n_sets, nc, rp));
  auto* b = new bote_batch();
  auto cleanup = [&](int code) {
    const std::string msg = g_err;  // (destroying the inner sweeps must not lose the text)
    bote_batch_destroy(b);
    g_err = msg;
    return code;
  };
  b->device = p->device;
  b->n = n;
  b->ns = ns;
  b->n_obj = n_obj;
  b->K = K;
  b->n_sets = n_sets;
  b->m = n_pinned;
  b->sets.resize(n_sets);
  for (uint32_t i = 0; i < n_sets; ++i) {
    bote::PinArgs& z = b->sets[i];
    z = bote::PinArgs{};
    z.pin_n = n_pinned;
    std::copy(pinned + (size_t)i * n_pinned, pinned + (size_t)(i + 1) * n_pinned, z.pin);
    std::sort(z.pin, z.pin + n_pinned);
    if (bounded) batch_limits(prev_s1 + 2 * (size_t)i, n, nc, rp->min_mean_decrease, rp->ft_metric, z.lim);
  }
  int rc;
  if (kernel != BOTE_KERNEL_GENERIC) {
    if ((rc = bote_sweep_create_pinned(p, servers, ns, clients, nc, n, pinned, n_pinned, objs, n_obj, K, rp, digest,
                                       kernel, &b->fast)))
      return cleanup(rc);
    if (b->fast->path != Path::Fast) {
      bote_sweep_destroy(b->fast);
      b->fast = nullptr;
    }
  }
  if ((rc = bote_sweep_create_pinned(p, servers, ns, clients, nc, n, pinned, n_pinned, objs, n_obj, K, rp, digest,
                                     BOTE_KERNEL_GENERIC, &b->gen)))
    return cleanup(rc);
  if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(BOTE_E_DEVICE, "hipSetDevice"));
  uint32_t cap = max_blocks;
  if (b->fast) {
    const int occ = bote::fast_occupancy(n, bote::FAST_PLAIN, bote::PIN_BATCH, b->fast->fshm);
    const uint32_t hw = (uint32_t)(device_cus(p->device) * occ);
    cap = cap ? std::min(cap, hw) : hw;
  }
  b->plan = batch_plan(ns, n, n_pinned, n_sets, cap);
  if (!b->plan.slices) return cleanup(fail(BOTE_E_RANGE, "the sets' rank space overflows 64 bits"));
  b->grid = (uint32_t)std::min<uint64_t>(b->plan.units, std::max<uint32_t>(cap, 1));
  if (b->result.alloc((size_t)n_sets * b->block_bytes()) != hipSuccess)
    return cleanup(fail(BOTE_E_NOMEM, "hipMalloc batch result blocks"));
  if (b->fast) {
    static_assert(bote::host::BATCH_MAX_SLICES == bote::BATCH_MAX_SLICES, "the host plan and the kernels agree on the slices");
    const size_t top_bytes = (size_t)n_sets * bote::BATCH_SET_LISTS * std::max<uint32_t>(n_obj, 1) * bote::KP * 16;
    if (b->dsets.alloc((size_t)n_sets * sizeof(bote::PinArgs)) != hipSuccess || b->top.alloc(top_bytes) != hipSuccess ||
        b->counters.alloc((size_t)n_sets * 16) != hipSuccess)
      return cleanup(fail(BOTE_E_NOMEM, "hipMalloc batch workspace"));
    // (all ones: the slots no unit and no fix-up writes are empty lists for the merge)
    if (hipMemcpy(b->dsets.p, b->sets.data(), (size_t)n_sets * sizeof(bote::PinArgs), hipMemcpyHostToDevice) !=
            hipSuccess ||
        hipMemset(b->top.p, 0xFF, top_bytes) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
      return cleanup(fail(BOTE_E_DEVICE, "upload batch tables"));
    if (hipEventCreate(&b->e0) != hipSuccess || hipEventCreate(&b->e1) != hipSuccess)
      return cleanup(fail(BOTE_E_DEVICE, "hipEventCreate"));
  }
  if (hipEventCreateWithFlags(&b->done, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(BOTE_E_DEVICE, "hipEventCreate"));
  *out = b;
  return BOTE_OK;
}

}  // namespace

extern "C" {

int bote_batch_create(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                      uint32_t n, const uint32_t* pinned, uint32_t n_sets, uint32_t n_pinned, uint32_t max_blocks,
                      const bote_objective* objs, uint32_t n_obj, uint32_t K, const bote_ranking_params* rp, int digest,
                      int kernel, bote_batch** out) {
  return batch_create(p, servers, ns, clients, nc, n, pinned, n_sets, n_pinned, max_blocks, objs, n_obj, K, rp, digest,
                      kernel, false, nullptr, out);
}

int bote_batch_create_bounded(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                              uint32_t nc, uint32_t n, const uint32_t* pinned, uint32_t n_sets, uint32_t n_pinned,
                              uint32_t max_blocks, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                              const bote_ranking_params* rp, int digest, int kernel, const uint64_t* prev_s1,
                              bote_batch** out) {
  return batch_create(p, servers, ns, clients, nc, n, pinned, n_sets, n_pinned, max_blocks, objs, n_obj, K, rp, digest,
                      kernel, true, prev_s1, out);
}

int bote_batch_limits(const bote_batch* b, uint32_t* out) {
  if (!b || !out) return fail(BOTE_E_ARG, "null argument");
  for (uint32_t i = 0; i < b->n_sets; ++i) std::copy(b->sets[i].lim, b->sets[i].lim + 2, out + 2 * (size_t)i);
  return BOTE_OK;
}

int bote_batch_launch(bote_batch* b, void* hip_stream) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!b) return fail(BOTE_E_ARG, "batch is null");
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const int rc = b->fast ? launch_batch_fast(b, st) : launch_per_set(b, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(b->done, st));
  b->launched = true;
  b->recomputed = false;
  return BOTE_OK;
}

int bote_batch_result(bote_batch* b, void* hip_stream, bote_topk_record* out, uint32_t* out_count,
                      uint64_t* out_valid, uint64_t* out_digest) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!b) return fail(BOTE_E_ARG, "batch is null");
  if (!b->launched) return fail(BOTE_E_ARG, "batch not launched");
  HIP_TRY(hipSetDevice(b->device));
  hipStream_t st = (hipStream_t)hip_stream;
  if (b->fast && !b->recomputed) {
    // a deferred config's full rank does not identify its set (a superset of
    // two sets defers for both), so there is no per-set fix-up: a batch that
    // deferred any config, or overflowed the queue, has every set recomputed
    // on the generic kernel (decided here, on the host)
    unsigned long long q = 0;
    HIP_TRY(hipMemcpyAsync(&q, b->fast->qcount.p, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (q > 0) {
      const int rc = launch_per_set(b, st);
      if (rc) return rc;
      HIP_TRY(hipEventRecord(b->done, st));
      b->recomputed = true;
    }
  }
  std::vector<uint8_t> blk((size_t)b->n_sets * b->block_bytes());
  HIP_TRY(hipMemcpyAsync(blk.data(), b->result.p, blk.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  static_assert(sizeof(bote_topk_record) == sizeof(TopkRecord), "record layout");
  for (uint32_t i = 0; i < b->n_sets; ++i)
    unpack_result(blk.data() + (size_t)i * b->block_bytes(), b->n_obj, b->K, bote::KP,
                  out ? (TopkRecord*)out + (size_t)i * b->n_obj * b->K : nullptr,
                  out_count ? out_count + (size_t)i * b->n_obj : nullptr, out_valid ? out_valid + i : nullptr,
                  out_digest ? out_digest + i : nullptr);
  return BOTE_OK;
}

int bote_batch_deferred(bote_batch* b, void* hip_stream, uint64_t* out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!b || !out) return fail(BOTE_E_ARG, "null argument");
  *out = 0;
  if (!b->fast || !b->launched) return BOTE_OK;
  HIP_TRY(hipSetDevice(b->device));
  unsigned long long q = 0;
  HIP_TRY(hipMemcpyAsync(&q, b->fast->qcount.p, 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  *out = q;
  return BOTE_OK;
}

int bote_batch_path(const bote_batch* b, int* out) {
  if (!b || !out) return fail(BOTE_E_ARG, "null argument");
  *out = b->fast ? (int)Path::Fast : (int)Path::Generic;
  return BOTE_OK;
}

int bote_batch_last_kernel_ms(bote_batch* b, float* out_ms) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!b || !out_ms) return fail(BOTE_E_ARG, "null argument");
  if (!b->launched) return fail(BOTE_E_ARG, "batch not launched");
  HIP_TRY(hipSetDevice(b->device));
  if (b->fast && !b->recomputed) {
    HIP_TRY(hipEventSynchronize(b->e1));
    HIP_TRY(hipEventElapsedTime(out_ms, b->e0, b->e1));
    return BOTE_OK;
  }
  uint32_t launches = 0;
  return bote_sweep_timing(b->gen, out_ms, &launches);
}

int bote_batch_plan(const bote_batch* b, uint32_t* out_slices, uint64_t* out_units, uint32_t* out_grid) {
  if (!b) return fail(BOTE_E_ARG, "batch is null");
  if (out_slices) *out_slices = b->plan.slices;
  if (out_units) *out_units = b->plan.units;
  if (out_grid) *out_grid = b->grid;
  return BOTE_OK;
}

int bote_batch_destroy(bote_batch* b) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!b) return BOTE_OK;
  (void)hipSetDevice(b->device);  // (kept in the handle: the planet may be gone)
  if (b->done) {
    if (b->launched) (void)hipEventSynchronize(b->done);
    (void)hipEventDestroy(b->done);
  }
  if (b->e0) (void)hipEventDestroy(b->e0);
  if (b->e1) (void)hipEventDestroy(b->e1);
  bote_sweep_destroy(b->fast);
  bote_sweep_destroy(b->gen);
  delete b;
  return BOTE_OK;
}

}  // extern "C"
