// bote_capi_census.hip — the census handle of the C ABI (include/bote_hip.h,
// bote_census_*): counts of the configs ranked before given records (DESIGN.md
// §4 "Census sweeps").  Host work only (bote_capi.hip's header).
//
// A census owns one sweep handle (bote_capi_sweep.hip) with K = 1 and no
// digest, built by the public entry on the path the census was routed to
// (census_route, bote_host.cpp), so that the uploads, the planet layouts, the
// kernels' arguments and the deferred queue are the sweep's own; the handle
// itself is never launched.  What the census adds is the threshold table, the
// counts (and the overflow fallback's own), the result block and the launch:
// the census variant of the fast kernel, the generic kernel's over the deferred
// rank list, its whole-range run gated on an overflowed queue, and the pick of
// the result, all stream-ordered.
#include "bote_capi.hpp"

using bote::EvalArgs;
using bote::Rec;
using Path = bote_sweep::Path;

using namespace bote::host;
using namespace bote::capi;

struct bote_census {
  using DBuf = bote::capi::DBuf;
  static constexpr uint32_t SLOTS = bote::MAXOBJ * bote::CENSUS_T;
  int device = 0;
  uint32_t n = 0, ns = 0, n_obj = 0;
  uint32_t T = 0;  // the last launch's
  bote_sweep* sw = nullptr;
  bool fast = false;
  uint32_t fgrid = 0, ggrid = 0;  // the census variants' persistent grids
  size_t fshm = 0;
  DBuf thr;                // [n_obj][T] records
  DBuf below, below_alt;   // [n_obj][T] counts: the fast pass and its fix-up (or the generic kernel); the fallback
  DBuf result;             // [n_obj x T counts][valid]
  hipEvent_t e0 = nullptr, e1 = nullptr, done = nullptr;
  bool launched = false;
};

namespace {

int launch_census(bote_census* c, uint64_t rb, uint64_t re, hipStream_t st) {
  const bote_sweep* s = c->sw;
  const uint32_t cells = c->n_obj * c->T;
  auto* counters = s->counters.as<unsigned long long>();
  bote::CensusArgs z{c->thr.as<Rec>(), c->T, c->below.as<unsigned long long>()};
  EvalArgs g = s->args;
  g.rb = rb;
  g.re = re;
  if (!c->fast) {
    g.runlen = sweep_runlen(re - rb, c->ggrid, s->bd);
    HIP_TRY(bote::launch_eval_census(g, c->n, z, c->ggrid, s->bd, s->shm, st, c->e0, c->e1));
    HIP_TRY(bote::launch_census_pick(z.below, nullptr, cells, counters, nullptr, nullptr, 0, c->result.as<uint64_t>(), st));
    return BOTE_OK;
  }
  auto* qcount = s->qcount.as<unsigned long long>();
  auto* counters_alt = s->counters_alt.as<unsigned long long>();
  const uint64_t cap = s->fargs.queue_cap;
  bote::FastArgs f = s->fargs;
  f.rb = rb;
  f.re = re;
  f.runlen = sweep_runlen(re - rb, c->fgrid, bote::FAST_BD);
  f.out_counters = counters;
  HIP_TRY(bote::launch_fast_census(f, c->n, z, c->fgrid, c->fshm, st, c->e0, c->e1));
  // the deferred configs, counted by nobody so far: the generic kernel over the
  // rank list, into the same counts (nothing when the queue overflowed)
  EvalArgs a = s->args;
  a.rank_list = s->queue.as<uint64_t>();
  a.rank_count = qcount;
  a.rb = 0;
  a.re = cap;
  a.runlen = 1;
  HIP_TRY(bote::launch_eval_census(a, c->n, z, s->xgrid, s->bd, s->shm, st));
  // overflow fallback: the whole range once on the generic kernel, into counts
  // of its own, decided on the device (every block exits at once otherwise);
  // the pick then discards the fast pass's counts
  g.runlen = sweep_runlen(re - rb, c->ggrid, s->bd);
  g.out_counters = counters_alt;
  g.run_if_over = qcount;
  g.over_cap = cap;
  bote::CensusArgs zf = z;
  zf.below = c->below_alt.as<unsigned long long>();
  HIP_TRY(bote::launch_eval_census(g, c->n, zf, c->ggrid, s->bd, s->shm, st));
  HIP_TRY(bote::launch_census_pick(z.below, zf.below, cells, counters, counters_alt, qcount, cap,
                                   c->result.as<uint64_t>(), st));
  return BOTE_OK;
}

}  // namespace

extern "C" {

int bote_census_create(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                       uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj,
                       const bote_ranking_params* rp, int kernel, bote_census** out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  bool has_score = false;
  if (!out) return fail(BOTE_E_ARG, "out is null");
  ARG_TRY(check_census_args(p ? p->R : 0, servers, ns, clients, nc, n, objs, n_obj, rp, kernel, has_score));
  const bool fair = has_score && rp && rp->min_fairness_fpaxos_improv != 0.0;
  int path = 0;
  ARG_TRY(census_route(fast_eligible(p->lat.data(), p->R, servers, ns, nc, fair), objs, n_obj, kernel, path));
  auto* c = new bote_census();
  auto cleanup = [&](int code) {
    const std::string msg = g_err;  // (destroying the inner sweep must not lose the text)
    bote_census_destroy(c);
    g_err = msg;
    return code;
  };
  c->device = p->device;
  c->n = n;
  c->ns = ns;
  c->n_obj = n_obj;
  int rc;
  if ((rc = bote_sweep_create_ex(p, servers, ns, clients, nc, n, objs, n_obj, 1, rp, 0,
                                 path ? BOTE_KERNEL_FAST : BOTE_KERNEL_GENERIC, &c->sw)))
    return cleanup(rc);
  if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(BOTE_E_DEVICE, "hipSetDevice"));
  const bote_sweep* s = c->sw;
  const int cus = device_cus(p->device);
  if (path && s->path == Path::Fast) {
    c->fshm = bote::fast_smem_bytes(s->fargs, n, bote::FAST_PLAIN, true);
    c->fgrid = (uint32_t)(cus * bote::fast_occupancy(n, bote::FAST_PLAIN, bote::PIN_NONE, c->fshm, true));
    c->fast = c->fgrid != 0;
  }
  if (path && !c->fast && kernel == BOTE_KERNEL_FAST)
    return cleanup(fail(BOTE_E_ARG, "the fast kernel does not fit this planet and client set (generic kernel)"));
  const int passes = bote::eval_passes(s->args.obj_kind, (int)n_obj);
  c->ggrid = (uint32_t)(cus * bote::eval_occupancy(n, false, s->bd, s->shm, false, passes, false, true));
  if (!c->ggrid) return cleanup(fail(BOTE_E_RANGE, "no census kernel for this config size"));
  if (c->thr.alloc(bote_census::SLOTS * 16) != hipSuccess || c->below.alloc(bote_census::SLOTS * 8) != hipSuccess ||
      c->below_alt.alloc(bote_census::SLOTS * 8) != hipSuccess ||
      c->result.alloc((bote_census::SLOTS + 1) * 8) != hipSuccess)
    return cleanup(fail(BOTE_E_NOMEM, "hipMalloc census workspace"));
  if (hipEventCreate(&c->e0) != hipSuccess || hipEventCreate(&c->e1) != hipSuccess ||
      hipEventCreateWithFlags(&c->done, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(BOTE_E_DEVICE, "hipEventCreate"));
  *out = c;
  return BOTE_OK;
}

int bote_census_launch(bote_census* c, const bote_topk_record* thr, uint32_t T, uint64_t rank_begin,
                       uint64_t rank_end, void* hip_stream) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!c) return fail(BOTE_E_ARG, "census is null");
  static_assert(sizeof(bote_topk_record) == sizeof(TopkRecord) && sizeof(TopkRecord) == sizeof(Rec), "record layout");
  static_assert(BOTE_CENSUS_MAX_THRESHOLDS == bote::CENSUS_T, "the header's limit is the kernels' table");
  ARG_TRY(check_census_launch((const TopkRecord*)thr, c->n_obj, T, c->ns, c->n, rank_begin, rank_end));
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const bote_sweep* s = c->sw;
  c->T = T;
  HIP_TRY(bote::launch_census_begin((const Rec*)thr, c->n_obj * T, c->thr.as<Rec>(), c->below.as<unsigned long long>(),
                                    c->fast ? c->below_alt.as<unsigned long long>() : nullptr,
                                    s->counters.as<unsigned long long>(),
                                    c->fast ? s->counters_alt.as<unsigned long long>() : nullptr,
                                    c->fast ? s->qcount.as<unsigned long long>() : nullptr, st));
  const int rc = launch_census(c, rank_begin, rank_end, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->done, st));
  c->launched = true;
  return BOTE_OK;
}

int bote_census_result(bote_census* c, void* hip_stream, uint64_t* out_below, uint64_t* out_valid) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!c) return fail(BOTE_E_ARG, "census is null");
  if (!c->launched) return fail(BOTE_E_ARG, "census not launched");
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t cells = c->n_obj * c->T;
  std::vector<uint64_t> blk(cells + 1);
  HIP_TRY(hipMemcpyAsync(blk.data(), c->result.p, blk.size() * 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  if (out_below) std::copy(blk.begin(), blk.begin() + cells, out_below);
  if (out_valid) *out_valid = blk[cells];
  return BOTE_OK;
}

int bote_census_deferred(bote_census* c, void* hip_stream, uint64_t* out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!c || !out) return fail(BOTE_E_ARG, "null argument");
  *out = 0;
  if (!c->fast || !c->launched) return BOTE_OK;
  HIP_TRY(hipSetDevice(c->device));
  unsigned long long q = 0;
  HIP_TRY(hipMemcpyAsync(&q, c->sw->qcount.p, 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  *out = q;
  return BOTE_OK;
}

int bote_census_path(const bote_census* c, int* out) {
  if (!c || !out) return fail(BOTE_E_ARG, "null argument");
  *out = c->fast ? (int)Path::Fast : (int)Path::Generic;
  return BOTE_OK;
}

int bote_census_last_kernel_ms(bote_census* c, float* out_ms) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!c || !out_ms) return fail(BOTE_E_ARG, "null argument");
  if (!c->launched) return fail(BOTE_E_ARG, "census not launched");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->e1));
  HIP_TRY(hipEventElapsedTime(out_ms, c->e0, c->e1));
  return BOTE_OK;
}

int bote_census_destroy(bote_census* c) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!c) return BOTE_OK;
  (void)hipSetDevice(c->device);  // (kept in the handle: the planet may be gone)
  // the last launch's work may still run on the census's and the inner sweep's
  // buffers: wait on its event, not on the caller's stream or the device
  if (c->done) {
    if (c->launched) (void)hipEventSynchronize(c->done);
    (void)hipEventDestroy(c->done);
  }
  if (c->e0) (void)hipEventDestroy(c->e0);
  if (c->e1) (void)hipEventDestroy(c->e1);
  bote_sweep_destroy(c->sw);
  delete c;
  return BOTE_OK;
}

}  // extern "C"
