// bote_capi.hip — C ABI (include/bote_hip.h) over the gfx950 kernels: the
// planet handle, the per-call entries and the chain search.  The sweep handle
// is bote_capi_sweep.hip, the multi-device search handle bote_capi_search.hip.
//
// Host responsibilities only: argument validation (the reference panics, we
// return BOTE_E_* codes; the checks are bote_host.cpp's), device buffers,
// launch geometry and the merge chain.  Every computation of latencies,
// quorums, leaders, histograms moments, scores and top-K selection runs on
// the device (the bote_*.hip kernel files).
#include "bote_capi.hpp"

using bote::EvalArgs;
using bote::SingleArgs;

using namespace bote::host;
using namespace bote::capi;

thread_local std::string bote::capi::g_err;

namespace {

// One call's view of its planet's cached workspaces (the caller holds the
// planet's mutex).  take() hands out the next one; a buffer the call does not
// want still uses up its slot, so every entry finds each of its buffers at
// the same slot whatever it was asked for, and a slot only ever grows.
struct Workspace {
  const bote_planet* p;
  hipStream_t st;
  size_t next = 0;
  Workspace(const bote_planet* planet) : p(planet), st(planet->stream) {}
  template <class T>
  hipError_t take(size_t count, T*& dev, bool wanted = true) {
    dev = nullptr;
    if (next == bote_planet::NWS) return hipErrorOutOfMemory;
    bote::capi::DBuf& b = p->ws[next++];
    if (!wanted) return hipSuccess;
    const hipError_t e = b.reserve(count * sizeof(T));
    if (e == hipSuccess) dev = b.as<T>();
    return e;
  }
  // take(), and the stream-ordered copy of `count` T to it
  template <class T>
  hipError_t upload(const T* host, size_t count, const T*& dev, bool wanted = true) {
    T* d = nullptr;
    const hipError_t e = take(count, d, wanted);
    dev = d;
    if (e != hipSuccess || !wanted || !count) return e;
    return hipMemcpyAsync(d, host, count * sizeof(T), hipMemcpyHostToDevice, st);
  }
};

// The optional outputs of one call: want() registers a host pointer once,
// "this many T, wanted under this condition", and gives the device pointer for
// the kernel's arguments (null when the caller passed none or the condition
// does not hold); copy_back() then copies exactly what was registered.
struct Outputs {
  struct Item {
    void *host, *dev;
    size_t bytes;
  };
  Workspace& ws;
  std::vector<Item> items;
  explicit Outputs(Workspace& w) : ws(w) {}
  template <class T>
  hipError_t want(T* host, size_t count, T*& dev, bool cond = true) {
    const hipError_t e = ws.take(count, dev, host && cond);
    if (dev) items.push_back(Item{host, dev, count * sizeof(T)});
    return e;
  }
  hipError_t copy_back() const {
    for (const Item& i : items) {
      const hipError_t e = hipMemcpyAsync(i.host, i.dev, i.bytes, hipMemcpyDeviceToHost, ws.st);
      if (e != hipSuccess) return e;
    }
    return hipSuccess;
  }
};

}  // namespace

extern "C" {

const char* bote_last_error(void) { return g_err.c_str(); }

int bote_device_count(int* out) {
  if (!out) return fail(BOTE_E_ARG, "out is null");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) c = 0;
  *out = c;
  return BOTE_OK;
}

// ------------------------------------------------------------------ planet
int bote_planet_create(const uint16_t* lat, uint32_t R, int device, bote_planet** out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!lat || !out) return fail(BOTE_E_ARG, "null argument");
  if (R == 0 || R > BOTE_MAX_REGIONS) return fail(BOTE_E_RANGE, "R must be in [1, 128]");
  for (size_t i = 0; i < (size_t)R * R; ++i)
    if (lat[i] > BOTE_MAX_LATENCY) return fail(BOTE_E_RANGE, "latency above 16383");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BOTE_E_NODEV, "no HIP device");
  if (device < 0 || device >= ndev) return fail(BOTE_E_ARG, "device out of range");
  HIP_TRY(hipSetDevice(device));
  auto* p = new bote_planet();
  p->device = device;
  p->R = R;
  p->lat.assign(lat, lat + (size_t)R * R);
  std::vector<uint32_t> m((size_t)R * R);
  for (size_t i = 0; i < m.size(); ++i) m[i] = (uint32_t)lat[i] << bote::LAT_SHIFT;
  if (hipMalloc(&p->d_mat, m.size() * 4) != hipSuccess) {
    delete p;
    return fail(BOTE_E_NOMEM, "hipMalloc planet");
  }
  if (hipMemcpy(p->d_mat, m.data(), m.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipFree(p->d_mat);
    delete p;
    return fail(BOTE_E_DEVICE, "upload planet / create its stream");
  }
  *out = p;
  return BOTE_OK;
}

int bote_planet_destroy(bote_planet* p) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!p) return BOTE_OK;
  (void)hipSetDevice(p->device);
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->d_mat) (void)hipFree(p->d_mat);
  if (p->stream) (void)hipStreamDestroy(p->stream);
  delete p;
  return BOTE_OK;
}

int bote_planet_regions(const bote_planet* p, uint32_t* out_R) {
  if (!p || !out_R) return fail(BOTE_E_ARG, "null argument");
  *out_R = p->R;
  return BOTE_OK;
}

// ---------------------------------------------------------------- protocol
int bote_quorum_size(int protocol, uint32_t n, uint32_t f) {
  switch (protocol) {
    case BOTE_FPAXOS: return (int)(f + 1);
    case BOTE_EPAXOS: { uint32_t m = n / 2; return (int)(m + (m + 1) / 2); }
    case BOTE_ATLAS: return (int)(n / 2 + f);
    case BOTE_TEMPO: return (int)(n / 2 + f);
    case BOTE_TEMPO_TINY: return (int)(2 * f);
    default: return fail(BOTE_E_ARG, "unknown protocol");
  }
}

uint32_t bote_max_f(uint32_t n) { return std::min(n / 2, 2u); }

uint64_t bote_binomial(uint32_t ns, uint32_t n) { return binom_u64(ns, n); }

int bote_percentile_index(uint32_t bp, uint32_t count, uint32_t* out_idx, int* out_whole) {
  uint32_t idx;
  bool whole;
  if (!out_idx || !out_whole) return fail(BOTE_E_ARG, "null argument");
  if (!percentile_index(bp, count, idx, whole)) return fail(BOTE_E_ARG, "percentile needs 1 <= bp <= 9999 and count >= 1");
  *out_idx = idx;
  *out_whole = whole ? 1 : 0;
  return BOTE_OK;
}

int bote_mean_decrease_limit(uint64_t prev_s1, uint32_t count, double min_mean_decrease, uint32_t* out_limit) {
  ARG_TRY(check_mean_limit_args(prev_s1, count, out_limit));
  *out_limit = mean_decrease_limit(prev_s1, count, min_mean_decrease);
  return BOTE_OK;
}

int bote_colex_unrank(uint64_t rank, uint32_t n, uint32_t ns, uint32_t* out) {
  if (!out || n > ns) return fail(BOTE_E_ARG, "bad unrank arguments");
  if (!colex_unrank(rank, n, ns, out)) return fail(BOTE_E_ARG, "rank out of range");
  return BOTE_OK;
}

// --------------------------------------------------- single configuration
// The fields every single-configuration launch fills, the server and client
// lists uploaded (the call's first two workspaces).
static int single_args(const bote_planet* p, Workspace& ws, const uint32_t* servers, uint32_t ns,
                       const uint32_t* clients, uint32_t nc, uint32_t q, SingleArgs& a) {
  a = SingleArgs{};
  a.mat = p->d_mat;
  a.R = p->R;
  HIP_TRY(ws.upload(servers, ns, a.servers));
  a.ns = ns;
  HIP_TRY(ws.upload(clients, nc, a.clients));
  a.nc = nc;
  a.q = q;
  return BOTE_OK;
}

static int run_single(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                      const uint32_t* froms, uint32_t nf, uint32_t q, uint32_t leader, int mode, uint64_t* out,
                      size_t nout) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!p || !out) return fail(BOTE_E_ARG, "null argument");
  ARG_TRY(check_single_args(p->R, servers, ns, clients, nc, froms, nf, q, leader, mode));
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->device));
  Workspace ws(p);
  SingleArgs a;
  int rc;
  if ((rc = single_args(p, ws, servers, ns, clients, nc, q, a))) return rc;
  HIP_TRY(ws.upload(froms, nf, a.froms));
  a.nf = nf;
  a.leader = leader;
  HIP_TRY(ws.take(nout, a.out));
  HIP_TRY(bote::launch_single(a, mode, ws.st));
  if (nout) HIP_TRY(hipMemcpyAsync(out, a.out, nout * 8, hipMemcpyDeviceToHost, ws.st));
  HIP_TRY(hipStreamSynchronize(ws.st));
  return BOTE_OK;
}

int bote_quorum_latencies(const bote_planet* p, const uint32_t* froms, uint32_t nf, const uint32_t* regions,
                          uint32_t nr, uint32_t q, uint64_t* out) {
  return run_single(p, regions, nr, nullptr, 0, froms, nf, q, 0, 0, out, nf);
}

int bote_leaderless(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                    uint32_t q, uint64_t* out) {
  return run_single(p, servers, ns, clients, nc, nullptr, 0, q, 0, 1, out, nc);
}

int bote_leader(const bote_planet* p, uint32_t leader, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                uint32_t nc, uint32_t q, uint64_t* out) {
  return run_single(p, servers, ns, clients, nc, nullptr, 0, q, leader, 2, out, nc);
}

int bote_all_leaders(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                     uint32_t q, uint64_t* out) {
  return run_single(p, servers, ns, clients, nc, nullptr, 0, q, 0, 3, out, (size_t)ns * nc);
}

int bote_best_leader(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                     uint32_t q, int stat, uint32_t* out_pos, uint64_t* out_lat) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!p || !out_pos) return fail(BOTE_E_ARG, "null argument");
  ARG_TRY(check_best_leader_args(p->R, servers, ns, clients, nc, q, stat));
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->device));
  Workspace ws(p);
  SingleArgs a;
  int rc;
  if ((rc = single_args(p, ws, servers, ns, clients, nc, q, a))) return rc;
  a.stat = stat;
  double* dstat = nullptr;
  HIP_TRY(ws.take((size_t)ns * nc, a.out));
  HIP_TRY(ws.take(ns, dstat));
  HIP_TRY(ws.take(1, a.out_pos));
  HIP_TRY(bote::launch_single(a, 3, ws.st));
  HIP_TRY(bote::launch_best_leader(a, a.out, dstat, ws.st));
  HIP_TRY(hipMemcpyAsync(out_pos, a.out_pos, 4, hipMemcpyDeviceToHost, ws.st));
  HIP_TRY(hipStreamSynchronize(ws.st));
  if (out_lat && nc) {
    HIP_TRY(hipMemcpyAsync(out_lat, a.out + (size_t)(*out_pos) * nc, nc * 8, hipMemcpyDeviceToHost, ws.st));
    HIP_TRY(hipStreamSynchronize(ws.st));
  }
  return BOTE_OK;
}

// ------------------------------------------------------------------- eval
// The work of a batch call on the device (the call's first four workspaces):
// the server and client lists, then the explicit configs or, without them,
// the binomial table the kernel unranks with.
struct Work {
  const uint32_t *srv = nullptr, *cli = nullptr, *cfgs = nullptr;
  const uint64_t* binom = nullptr;
  std::vector<uint64_t> table;  // kept alive: the async upload reads it
};
static int upload_work(Workspace& ws, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                       uint32_t n, const uint32_t* configs, uint64_t ncfg, Work& w) {
  HIP_TRY(ws.upload(servers, ns, w.srv));
  HIP_TRY(ws.upload(clients, nc, w.cli));
  HIP_TRY(ws.upload(configs, ncfg * n, w.cfgs, configs != nullptr));
  if (!configs) w.table = binom_table(ns, n);
  HIP_TRY(ws.upload(w.table.data(), w.table.size(), w.binom, !configs));
  return BOTE_OK;
}

static int eval_impl(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                     uint32_t nc, uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                     const bote_ranking_params* rp, uint32_t keys, uint32_t* out_vals, uint32_t* out_leader,
                     uint64_t* out_sum, uint64_t* out_sumsq, double* out_mean, double* out_cov, double* out_score,
                     uint8_t* out_valid, uint64_t* out_al_sum, uint64_t* out_al_sumsq) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  ARG_TRY(check_eval_args(p ? p->R : 0, servers, ns, clients, nc, n, configs, rank_begin, ncfg, rp, keys));
  if (ncfg == 0) return BOTE_OK;
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->device));
  Workspace ws(p);
  Work w;
  int rc;
  if ((rc = upload_work(ws, servers, ns, clients, nc, n, configs, ncfg, w))) return rc;
  EvalArgs a{};
  a.mat = p->d_mat;
  a.R = p->R;
  a.srv = w.srv;
  a.ns = ns;
  a.cli = w.cli;
  a.nc = nc;
  a.srv_sorted = std::is_sorted(servers, servers + ns) ? 1 : 0;
  a.cfgs = w.cfgs;
  a.binom = w.binom;
  a.rb = configs ? 0 : rank_begin;
  a.re = a.rb + ncfg;
  a.runlen = 1;
  a.keys = keys;
  fill_rank_params(a, rp);
  const size_t stride = 5ull * nc + 5ull * n;
  const size_t NS = keys ? BOTE_NSLOTS_X : bote::NSLOT;
  const size_t nal = (size_t)ncfg * 2 * n;
  Outputs outs(ws);
  HIP_TRY(outs.want(out_vals, ncfg * stride, a.out_vals));
  HIP_TRY(outs.want(out_leader, ncfg, a.out_leader));
  HIP_TRY(outs.want(out_sum, ncfg * NS, a.out_s1));
  HIP_TRY(outs.want(out_sumsq, ncfg * NS, a.out_s2));
  HIP_TRY(outs.want(out_mean, ncfg * NS, a.out_mean));
  HIP_TRY(outs.want(out_cov, ncfg * NS, a.out_cov));
  HIP_TRY(outs.want(out_score, ncfg, a.out_score, rp != nullptr));
  HIP_TRY(outs.want(out_valid, ncfg, a.out_valid, rp != nullptr));
  HIP_TRY(outs.want(out_al_sum, nal, a.out_al_s1, keys != 0));
  HIP_TRY(outs.want(out_al_sumsq, nal, a.out_al_s2, keys != 0));

  const uint32_t bd = 256;
  size_t shm = bote::eval_smem_bytes(a, n, bd, false);
  if (shm > device_max_lds(p->device)) return fail(BOTE_E_RANGE, "planet/client set too large for LDS");
  int nb = bote::eval_occupancy(n, true, bd, shm, keys != 0);
  uint64_t want = (ncfg + bd - 1) / bd;
  uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)device_cus(p->device) * nb);
  HIP_TRY(bote::launch_eval(a, n, true, grid, bd, shm, ws.st));
  HIP_TRY(outs.copy_back());
  HIP_TRY(hipStreamSynchronize(ws.st));
  return BOTE_OK;
}

int bote_eval(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
              uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg, const bote_ranking_params* rp,
              uint32_t* out_vals, uint32_t* out_leader, uint64_t* out_sum, uint64_t* out_sumsq, double* out_mean,
              double* out_cov, double* out_score, uint8_t* out_valid) {
  return eval_impl(p, servers, ns, clients, nc, n, configs, rank_begin, ncfg, rp, 0, out_vals, out_leader, out_sum,
                   out_sumsq, out_mean, out_cov, out_score, out_valid, nullptr, nullptr);
}

int bote_eval_keys(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients, uint32_t nc,
                   uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg, uint32_t keys,
                   uint32_t* out_leader, uint64_t* out_sum, uint64_t* out_sumsq, uint64_t* out_al_sum,
                   uint64_t* out_al_sumsq) {
  return eval_impl(p, servers, ns, clients, nc, n, configs, rank_begin, ncfg, nullptr, keys, nullptr, out_leader,
                   out_sum, out_sumsq, nullptr, nullptr, nullptr, nullptr, out_al_sum, out_al_sumsq);
}

// ------------------------------------------ leaderless, many quorum sizes
// Bote::leaderless (lib.rs:38-59) over a batch of configurations for each of
// `nq` quorum sizes: Tempo's fast (n/2 + f; tiny 2f) and write (f + 1)
// quorums (fantoch/src/config.rs:317-329), which compute_stats does not key.
int bote_eval_leaderless(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                         uint32_t nc, uint32_t n, const uint32_t* configs, uint64_t rank_begin, uint64_t ncfg,
                         const uint32_t* quorum_sizes, uint32_t nq, uint32_t* out_vals, uint64_t* out_sum,
                         uint64_t* out_sumsq) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  ARG_TRY(check_leaderless_args(p ? p->R : 0, servers, ns, clients, nc, n, configs, rank_begin, ncfg, quorum_sizes,
                                nq));
  if (ncfg == 0) return BOTE_OK;
  std::lock_guard<std::mutex> lk(p->mu);
  HIP_TRY(hipSetDevice(p->device));
  Workspace ws(p);
  Work w;
  int rc;
  if ((rc = upload_work(ws, servers, ns, clients, nc, n, configs, ncfg, w))) return rc;
  bote::LqArgs a{};
  a.mat = p->d_mat;
  a.R = p->R;
  a.srv = w.srv;
  a.ns = ns;
  a.cli = w.cli;
  a.nc = nc;
  HIP_TRY(ws.upload(quorum_sizes, nq, a.qs));
  a.nq = nq;
  a.ncfg = ncfg;
  a.cfgs = w.cfgs;
  a.binom = w.binom;
  if (!configs) a.rank_begin = rank_begin;
  const size_t nv = (size_t)ncfg * nq * (nc + n), nm = (size_t)ncfg * nq * 2;
  Outputs outs(ws);
  HIP_TRY(outs.want(out_vals, nv, a.out_vals));
  HIP_TRY(outs.want(out_sum, nm, a.out_sum));
  HIP_TRY(outs.want(out_sumsq, nm, a.out_sumsq));
  const size_t shm = bote::lq_smem_bytes(a, n);
  if (shm > device_max_lds(p->device)) return fail(BOTE_E_RANGE, "planet/client set too large for LDS");
  const uint32_t grid = (uint32_t)std::min<uint64_t>((ncfg + 255) / 256, (uint64_t)device_cus(p->device) * 4);
  HIP_TRY(bote::launch_leaderless_q(a, n, grid, shm, ws.st));
  HIP_TRY(outs.copy_back());
  HIP_TRY(hipStreamSynchronize(ws.st));
  return BOTE_OK;
}

// ---------------------------------------- superset chains (ranking product)
int bote_evolving_chains(int device, uint32_t ns, const uint32_t* counts, const uint64_t* const* masks,
                         const double* const* scores, const double* const* means, double min_mean_decrease,
                         int ft_metric, uint64_t max_out, uint32_t* out_idx, double* out_score, uint64_t* out_total) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!counts || !masks || !scores || !means || !out_total) return fail(BOTE_E_ARG, "null argument");
  if (ns == 0 || ns > 64) return fail(BOTE_E_RANGE, "the server list must hold 1 to 64 regions");
  ARG_TRY(check_ft_metric(ft_metric));
  if (max_out && (!out_idx || !out_score)) return fail(BOTE_E_ARG, "null output");
  ARG_TRY(check_chain_levels(ns, counts, masks, scores, means));
  bote::ChainHostLevel lv[6];
  for (uint32_t l = 0; l < 6; ++l) lv[l] = bote::ChainHostLevel{counts[l], 3 + 2 * l, masks[l], scores[l], means[l]};
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(BOTE_E_NODEV, "no HIP device");
  if (device < 0 || device >= ndev) return fail(BOTE_E_ARG, "device out of range");
  HIP_TRY(hipSetDevice(device));
  hipStream_t st = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int too_many = 0;
  hipError_t e = bote::chain_search(lv, ns, ft_metric, min_mean_decrease, max_out, out_idx, out_score, out_total, st,
                                    &too_many);
  (void)hipStreamDestroy(st);
  if (e != hipSuccess) return fail(BOTE_E_DEVICE, std::string("chain search: ") + hipGetErrorString(e));
  if (too_many) return fail(BOTE_E_RANGE, "more than 2^31 chain prefixes at one level");
  return BOTE_OK;
}

// test entry, not part of the ABI: launch_seed over caller-supplied keys
// (keys: n_obj rows of nsamp, row o at keys[o * nsamp]; out: n_obj keys)
int bote_test_seed(int device, const uint64_t* keys, uint32_t nsamp, uint32_t n_obj, uint32_t K, uint64_t* out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!keys || !out || nsamp == 0 || n_obj == 0) return fail(BOTE_E_ARG, "bad seed test arguments");
  if (n_obj > (uint32_t)bote::MAXOBJ) return fail(BOTE_E_RANGE, "at most 8 rows per seed launch");
  HIP_TRY(hipSetDevice(device));
  DBuf din, dout;
  const size_t nb = (size_t)n_obj * nsamp * 8;
  if (din.alloc(nb) != hipSuccess || dout.alloc((size_t)n_obj * 8) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc seed test buffers");
  HIP_TRY(hipMemcpy(din.p, keys, nb, hipMemcpyHostToDevice));
  HIP_TRY(bote::launch_seed(din.as<uint64_t>(), nsamp, n_obj, K, dout.as<uint64_t>(), nullptr));
  HIP_TRY(hipMemcpy(out, dout.p, (size_t)n_obj * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipDeviceSynchronize());
  return BOTE_OK;
}

// test entry, not part of the ABI: the list merges over caller-supplied record
// slots (tests/test_gpu_merge.py).  src: n_lists x n_obj x KP records (key,
// rank), list i of objective o at record (i * n_obj + o) * KP, every slot the
// caller's (what follows a terminator too); alt: the same for alt_lists lists,
// or null with 0; kbound: n_obj keys or null; sel: one word or null (the
// device reads alt and counters_alt when *sel > cap); counters, counters_alt:
// two words each.  mode 0: merge_lists, a sweep's merge chain (one wide launch
// when kbound && sel and both counts <= WIDE_MERGE_LISTS, else the tree down
// to one list, and the counters); 1: launch_merge_wide; 2: one launch_merge
// level with `out_stride` records between its output lists.  out: the result
// lists, all KP slots of every objective (modes 0 and 1: one list; mode 2:
// ceil(max(n_lists, alt_lists) / 8) lists, packed n_obj x KP apart);
// out_counters: the result's two counters (mode 2 writes none).  The device
// result is preset to bytes of 0xAB: a slot no kernel wrote shows as that.
int bote_test_merge(int device, int mode, const uint64_t* src, uint32_t n_lists, const uint64_t* alt,
                    uint32_t alt_lists, uint32_t n_obj, uint32_t K, const uint64_t* kbound, const uint64_t* sel,
                    uint64_t cap, const uint64_t* counters, const uint64_t* counters_alt, uint64_t out_stride,
                    uint64_t* out, uint64_t* out_counters) {
  using bote::Rec;
  DevGuard dev_guard;  // the caller's current device is restored on return
  constexpr uint32_t TREE_LISTS_MAX = 1u << 16;
  if (!src || !counters || !out || !out_counters || n_lists == 0) return fail(BOTE_E_ARG, "bad merge test arguments");
  if ((alt != nullptr) != (alt_lists != 0)) return fail(BOTE_E_ARG, "alt and alt_lists go together");
  if (sel && (!alt || !counters_alt)) return fail(BOTE_E_ARG, "sel needs alt and counters_alt");
  if (mode < 0 || mode > 2) return fail(BOTE_E_ARG, "merge test mode is 0 (chain), 1 (wide) or 2 (one tree level)");
  if (n_obj == 0 || n_obj > (uint32_t)bote::MAXOBJ) return fail(BOTE_E_RANGE, "1 to 8 objectives per merge");
  if (K == 0 || K > (uint32_t)bote::KP) return fail(BOTE_E_RANGE, "K is 1 to KP");
  if (n_lists > TREE_LISTS_MAX || alt_lists > TREE_LISTS_MAX) return fail(BOTE_E_RANGE, "at most 65536 lists");
  if (mode == 1 && (n_lists > bote::WIDE_MERGE_LISTS || alt_lists > bote::WIDE_MERGE_LISTS))
    return fail(BOTE_E_RANGE, "at most 4096 lists in one wide merge");
  const uint64_t lstride = (uint64_t)n_obj * bote::KP;
  if (mode == 2 && (out_stride < lstride || out_stride > 4 * lstride))
    return fail(BOTE_E_RANGE, "out_stride is 1 to 4 list strides");
  HIP_TRY(hipSetDevice(device));
  const uint32_t groups = (std::max(n_lists, alt_lists) + bote::G_MERGE_LISTS - 1) / bote::G_MERGE_LISTS;
  const size_t list_bytes = (size_t)lstride * 16, tmp_bytes = (size_t)groups * list_bytes;
  const size_t res_bytes = mode == 2 ? (size_t)groups * out_stride * 16 : list_bytes + 16;
  DBuf dsrc, dalt, dkb, dsel, dc, dca, tmp0, tmp1, res;
  if (dsrc.alloc(n_lists * list_bytes) != hipSuccess || dalt.alloc(alt_lists * list_bytes) != hipSuccess ||
      dkb.alloc(bote::MAXOBJ * 8) != hipSuccess || dsel.alloc(8) != hipSuccess || dc.alloc(16) != hipSuccess ||
      dca.alloc(16) != hipSuccess || tmp0.alloc(tmp_bytes) != hipSuccess || tmp1.alloc(tmp_bytes) != hipSuccess ||
      res.alloc(res_bytes) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc merge test buffers");
  HIP_TRY(hipMemcpy(dsrc.p, src, n_lists * list_bytes, hipMemcpyHostToDevice));
  if (alt) HIP_TRY(hipMemcpy(dalt.p, alt, alt_lists * list_bytes, hipMemcpyHostToDevice));
  if (kbound) HIP_TRY(hipMemcpy(dkb.p, kbound, (size_t)n_obj * 8, hipMemcpyHostToDevice));
  if (sel) HIP_TRY(hipMemcpy(dsel.p, sel, 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(dc.p, counters, 16, hipMemcpyHostToDevice));
  if (counters_alt) HIP_TRY(hipMemcpy(dca.p, counters_alt, 16, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(tmp0.p, 0xAB, tmp_bytes));
  HIP_TRY(hipMemset(tmp1.p, 0xAB, tmp_bytes));
  HIP_TRY(hipMemset(res.p, 0xAB, res_bytes));
  const Rec* a = alt ? dalt.as<Rec>() : nullptr;
  const unsigned long long* kb = kbound ? dkb.as<unsigned long long>() : nullptr;
  const unsigned long long* sl = sel ? dsel.as<unsigned long long>() : nullptr;
  const unsigned long long* ca = counters_alt ? dca.as<unsigned long long>() : nullptr;
  uint64_t* cdst = (uint64_t*)((char*)res.p + list_bytes);
  if (mode == 0) {
    int rc = merge_lists(dsrc.as<Rec>(), n_lists, a, alt_lists, lstride, sl, cap, kb, tmp0.as<Rec>(), tmp1.as<Rec>(),
                         res.p, n_obj, K, dc.as<unsigned long long>(), ca, nullptr);
    if (rc) return rc;
  } else if (mode == 1) {
    HIP_TRY(bote::launch_merge_wide(dsrc.as<Rec>(), n_lists, a, alt_lists, lstride, sl, cap, kb, res.as<Rec>(), n_obj, K,
                                    dc.as<unsigned long long>(), ca, cdst, nullptr));
  } else {
    HIP_TRY(bote::launch_merge(dsrc.as<Rec>(), n_lists, a, alt_lists, lstride, sl, cap, res.as<Rec>(), out_stride,
                               n_obj, nullptr));
  }
  HIP_TRY(hipDeviceSynchronize());
  if (mode == 2) {
    HIP_TRY(hipMemcpy2D(out, list_bytes, res.p, (size_t)out_stride * 16, list_bytes, groups, hipMemcpyDeviceToHost));
  } else {
    HIP_TRY(hipMemcpy(out, res.p, list_bytes, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_counters, cdst, 16, hipMemcpyDeviceToHost));
  }
  return BOTE_OK;
}

}  // extern "C"
