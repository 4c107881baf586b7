// bote_capi_sweep.hip — the sweep handle of the C ABI (include/bote_hip.h):
// bote_sweep_create* (planning glue over bote_host.cpp, device buffers), the
// per-range chunk and seed tables, a launch with its merge chain, results and
// timing, and bote_merge_device.  Host work only (bote_capi.hip's header).
#include <cstdlib>

#include "bote_capi.hpp"

using bote::EvalArgs;
using bote::Rec;
using Path = bote_sweep::Path;

using namespace bote::host;
using namespace bote::capi;

namespace {
constexpr uint64_t QUEUE_CAP = 1ull << 20;  // deferred near-tie configs per launch

#ifndef BOTE_CHUNKS_PER_WAVE
#define BOTE_CHUNKS_PER_WAVE 32
#endif
// least client count for the member-binned loop on the base key set (a build
// knob for A/B timing builds only; scripts/build_variant.sh)
#ifndef BOTE_GBINS_MIN_NC
#define BOTE_GBINS_MIN_NC 32
#endif
}  // namespace

extern "C" {

int bote_sweep_create(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                      uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                      const bote_ranking_params* rp, int digest, bote_sweep** out) {
  return bote_sweep_create_ex(p, servers, ns, clients, nc, n, objs, n_obj, K, rp, digest, BOTE_KERNEL_AUTO, out);
}

int bote_sweep_create_ex(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                         uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                         const bote_ranking_params* rp, int digest, int kernel, bote_sweep** out) {
  return bote_sweep_create_keys(p, servers, ns, clients, nc, n, objs, n_obj, K, rp, digest, kernel, 0, out);
}

// bote_sweep_create_keys in steps.  Each returns a BOTE_E_* code (the entry
// point destroys the half-built sweep on a failure); the pure arithmetic
// behind them is bote_host.cpp's (fast_limits, score_bands, ...).  Step 1,
// before anything is allocated, is its argument check (check_sweep_args).

// A percentile objective as the kernels take it (bote_kernels.hpp OBJ_PCTL):
// which of the slot's largest values, and whether its neighbour is added,
// from bp and the slot's count (check_sweep_args admitted both).
static uint32_t pctl_device_kind(uint32_t bp, uint32_t count) {
  uint32_t idx = 0;
  bool whole = false;
  percentile_index(bp, count, idx, whole);
  // idx == 0 is the least value itself (x = p * count > 0 is then no integer)
  return bote::OBJ_PCTL | (whole && idx ? bote::PCTL_WHOLE : 0u) | percentile_need(bp, count);
}
static_assert(PCTL_MAX_NEED == (uint32_t)bote::PCTL_DEPTH && bote::PCTL_DEPTH <= (int)bote::PCTL_NEED_MASK,
              "the admitted need fits the generic kernel's list and the encoding");

// Step 2: the server, client and binomial lists on the device, the generic
// kernel's arguments (s->args) and its launch geometry.
// (objs: the n_obj key entries, a constrained sweep's constraints after its objectives)
static int sweep_upload_lists(bote_sweep* s, const uint32_t* servers, const uint32_t* clients,
                              const bote_objective* objs, uint32_t n_obj, const bote_ranking_params* rp,
                              bool has_score, int digest, uint32_t keys) {
  const bote_planet* p = s->p;
  const uint32_t n = s->n, ns = s->ns, nc = s->nc;
  EvalArgs& a = s->args;
  a = EvalArgs{};
  auto t = binom_table(ns, n);
  if (s->srv.alloc(ns * 4) != hipSuccess || s->cli.alloc(nc * 4) != hipSuccess ||
      s->binom.alloc(t.size() * 8) != hipSuccess || s->counters.alloc(16) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc sweep lists");
  if (hipMemcpy(s->srv.p, servers, ns * 4, hipMemcpyHostToDevice) != hipSuccess ||
      (nc && hipMemcpy(s->cli.p, clients, nc * 4, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemcpy(s->binom.p, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(BOTE_E_DEVICE, "upload sweep lists");
  a.mat = p->d_mat;
  a.R = p->R;
  a.srv = s->srv.as<uint32_t>();
  a.ns = ns;
  a.cli = s->cli.as<uint32_t>();
  a.nc = nc;
  a.srv_sorted = std::is_sorted(servers, servers + ns) ? 1 : 0;
  a.binom = s->binom.as<uint64_t>();
  fill_rank_params(a, has_score ? rp : nullptr);
  a.n_obj = (int)n_obj;
  for (uint32_t o = 0; o < n_obj; ++o) {
    a.obj_kind[o] = is_percentile_kind(objs[o].kind)
                        ? pctl_device_kind(objs[o].kind & 0xFFFF, slot_count(objs[o].slot, nc, n))
                        : objs[o].kind;
    a.obj_slot[o] = objs[o].slot;
  }
  a.K = s->K;
  a.want_digest = digest ? 1 : 0;
  a.keys = keys;
  a.out_counters = s->counters.as<unsigned long long>();

  s->bd = 256;
  a.out_top = (Rec*)1;  // sizing with top-K structures
  s->shm = bote::eval_smem_bytes(a, n, s->bd, true);
  a.out_top = nullptr;
  if (s->shm > device_max_lds(p->device)) return fail(BOTE_E_RANGE, "planet/client set too large for LDS");
  const int passes = bote::eval_passes(a.obj_kind, (int)n_obj);
  int nb = bote::eval_occupancy(n, false, s->bd, s->shm, keys != 0, passes, s->pz.pin_n != 0, false, s->n_con != 0);
  s->grid = (uint32_t)(device_cus(p->device) * nb);
  s->xgrid = 32;
  return BOTE_OK;
}

// The group kernel's geometry at one workgroup size: the position table (n <=
// 7) unless its LDS lowers the workgroups per CU, then as many client lines
// per wave (<= 16) as keep that occupancy.  A workgroup shares the
// client-quad matrix (CQT) among its waves, so at R = 128 larger workgroups
// leave LDS for the client lines that 256-thread ones cannot hold (a step has
// 7.7 distinct (p1, p2) on average at R=64 n=7, 4.0 at R=128 n=6; DESIGN.md
// §4).  `f` is the candidate: a copy of the sweep's arguments, with gbins set.
struct GGeo {
  uint32_t bd = 0, grx = 0, gslots = 0, gqsh = 10;
  int occ = 0;
  size_t shm = 0;
};
static GGeo group_geometry(bote::FastArgs f, uint32_t n, bool def_obj, uint32_t bd, size_t max_lds) {
  f.gbd = bd;
  // qtab member planes (non-PERM kernels): one u32 per thread, so the
  // plane stride 1 << gqsh must hold gbd * 4 bytes (bote_group.hip)
  f.gqsh = 10;
  while ((1u << f.gqsh) < f.gbd * 4) ++f.gqsh;
  f.gslots = 0;
  f.grx = 0;
  if (bote::group_uses_lines(n)) {
    const int occ_plain = bote::group_occupancy(f, n, bote::group_smem_bytes(f, n), def_obj);
    f.grx = 1;
    if (bote::group_occupancy(f, n, bote::group_smem_bytes(f, n), def_obj) < occ_plain) f.grx = 0;
    const int occ0 = bote::group_occupancy(f, n, bote::group_smem_bytes(f, n), def_obj);
    for (uint32_t sl = 16; sl >= 1; --sl) {
      f.gslots = sl;
      const size_t sh = bote::group_smem_bytes(f, n);
      if (sh <= max_lds && bote::group_occupancy(f, n, sh, def_obj) >= occ0) break;
      f.gslots = 0;
    }
  }
  GGeo g{bd, f.grx, f.gslots, f.gqsh, 0, bote::group_smem_bytes(f, n)};
  if (g.shm <= max_lds) g.occ = bote::group_occupancy(f, n, g.shm, def_obj);
  return g;
}

// The best geometry over the candidate workgroup sizes (pick_group_geometry;
// occ == 0: none fits): multiples of 256 threads up to 1024 (the extended key
// set's kernels are bounded to bote::group_supports_keys' size).  Sizes of 6
// or 10 waves put unequal wave counts on the 4 SIMDs of a CU (384 threads
// measured 16-21 % slower than both neighbours; more waves per SIMD is not
// the aim either: R=128 n=6 at 640 threads, 5 waves/SIMD, 369 ms vs 348 ms at
// 256 threads, 2 waves/SIMD).  BOTE_GROUP_BD (env) forces one
// size (A/B timing).
static GGeo best_group_geometry(const bote::FastArgs& f, uint32_t n, bool def_obj, size_t max_lds) {
  const char* bd_env = getenv("BOTE_GROUP_BD");
  const uint32_t bd_only = bd_env ? (uint32_t)strtoul(bd_env, nullptr, 0) : 0u;
  GGeo best;
  for (uint32_t bd = 256; bd <= 1024; bd += 128) {
    if (bd_only ? bd != bd_only : bd % 256 != 0) continue;
    if (f.keys && !bote::group_supports_keys(n, bd)) continue;
    const GGeo g = group_geometry(f, n, def_obj, bd, max_lds);
    if (g.occ > 0 && pick_group_geometry(g.bd, g.occ, g.gslots, best.bd, best.occ, best.gslots)) best = g;
  }
  return best;
}

// Step 4 (a fast sweep): the group kernel when wanted and it fits: n >= 4,
// positions fit 8 bits, and (AUTO) enough lane utilisation.
static int sweep_plan_group(bote_sweep* s, const FastLimits& lim, bool compiled_objs, int kernel) {
  const bote_planet* p = s->p;
  const uint32_t n = s->n, ns = s->ns, nc = s->nc;
  bote::FastArgs& f = s->fargs;
  // (a MAX, percentile or MDTM objective: the fast kernel's variant, s->tail; a
  // forced group kernel was refused with the arguments, check_sweep_args)
  // (nor a constrained sweep: the group kernel does not apply constraints)
  bool want_group = n >= 4 && ns <= 256 && group_utilisation(ns, n) >= 0.9 && !s->tail && !s->pz.pin_n && !s->n_con;
  if (kernel != BOTE_KERNEL_AUTO) want_group = n >= 4 && ns <= 256 && kernel == BOTE_KERNEL_GROUP;
  if (kernel == BOTE_KERNEL_GROUP && !want_group) return fail(BOTE_E_ARG, "group kernel needs n >= 4");
  if (s->path == Path::Generic || !want_group) return BOTE_OK;
  auto lt = low_table(ns - (n - 3));
#ifdef BOTE_DEBUG
  f.lowtab_n = lt.size();
#endif
  // (64 padding entries: a step's lanes read the table past a group's
  // last row without a clamp; those lanes hold no config)
  lt.resize(lt.size() + 64, 0u);
  if (s->lowtab.alloc(std::max<size_t>(lt.size(), 1) * 4) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc group low table");
  if (!lt.empty() && hipMemcpy(s->lowtab.p, lt.data(), lt.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
    return fail(BOTE_E_DEVICE, "upload group low table");
  f.lowtab = s->lowtab.as<uint32_t>();
  // the objective set compiled into the DEF kernels (bote.py
  // DEFAULT_OBJECTIVES; with the extended keys, CONFIG5_OBJECTIVES)
  s->def_obj = compiled_objs && f.want_score;
  // the member-binned client loop on the base key set: bench-shaped
  // sweeps (server identity, digest, F1F2: the SI kernels) with >= 32
  // clients, where the bin fields cannot overflow (R=64 n=7: 14.26 vs
  // 14.89 ms for the register lookups, profiles/r04c; R=128 n=6: 168 vs
  // 180 ms, round 3)
  f.gbins = !f.keys && s->def_obj && bote::group_uses_lines(n) && nc >= BOTE_GBINS_MIN_NC && lim.bins_ok &&
            f.srv_identity && f.want_digest && f.ft_metric == 2;
  const GGeo best = best_group_geometry(f, n, s->def_obj, device_max_lds(p->device));
  if (best.occ > 0 && (!f.keys || s->def_obj)) {
    f.gbd = best.bd;
    f.grx = best.grx;
    f.gslots = best.gslots;
    f.gqsh = best.gqsh;
    s->path = Path::Group;
    s->fshm = best.shm;
    s->fgrid = (uint32_t)(device_cus(p->device) * best.occ);
  }
  return BOTE_OK;
}

// The fast kernels' arguments (s->fargs): the client-quad layouts, uploaded
// (column sums are computed on the device), and the host plan copied in.
static int fill_fast_args(bote_sweep* s, const uint32_t* servers, const uint32_t* clients, const FastLimits& lim) {
  const bote_planet* p = s->p;
  const EvalArgs& a = s->args;
  const uint32_t ns = s->ns, nc = s->nc;
  bote::FastArgs& f = s->fargs;
  f = bote::FastArgs{};
  std::vector<uint32_t> ident(p->R);
  for (uint32_t i = 0; i < p->R; ++i) ident[i] = i;
  bool cli_ident = nc == p->R && std::equal(clients, clients + nc, ident.begin());
  uint32_t cq_quads = 0, rq_quads = 0, cq_stride = 0, rq_stride = 0;
  auto cq = quad_layout(p->lat.data(), p->R, clients, nc, bote::LAT_SHIFT, cq_quads, cq_stride);
  std::vector<uint16_t> rq;
  if (!cli_ident) rq = quad_layout(p->lat.data(), p->R, ident.data(), p->R, bote::LAT_SHIFT, rq_quads, rq_stride);
  if (s->cqt.alloc(cq.size() * 2) != hipSuccess || (!cli_ident && s->rqt.alloc(rq.size() * 2) != hipSuccess) ||
      s->queue.alloc(QUEUE_CAP * 8) != hipSuccess || s->qcount.alloc(16) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc fast-path buffers");
  if (hipMemcpy(s->cqt.p, cq.data(), cq.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
      (!cli_ident && hipMemcpy(s->rqt.p, rq.data(), rq.size() * 2, hipMemcpyHostToDevice) != hipSuccess))
    return fail(BOTE_E_DEVICE, "upload fast-path layouts");
  f.cqt = s->cqt.as<uint2>();
  f.rqt = cli_ident ? s->cqt.as<uint2>() : s->rqt.as<uint2>();
  f.rq_separate = cli_ident ? 0 : 1;
  f.R = p->R;
  f.cq_quads = cq_quads;
  f.rq_quads = cli_ident ? cq_quads : rq_quads;
  f.cq_stride = cq_stride;
  f.rq_stride = cli_ident ? cq_stride : rq_stride;
  f.srv = s->srv.as<uint32_t>();
  f.ns = ns;
  f.keys = a.keys;
  f.srv_identity = 1;
  for (uint32_t i = 0; i < ns; ++i) f.srv_identity &= servers[i] == i;
  f.nc = nc;
  f.binom = s->binom.as<uint64_t>();
  f.s2_flush = lim.s2_flush;
  f.g_flush = lim.g_flush;
  f.k_flush = lim.k_flush;
  f.s32 = lim.s32 ? 1u : 0u;
  f.v32 = lim.v32 ? 1u : 0u;
  f.want_score = a.want_score;
  f.p_fmean = a.p_fmean;
  f.p_emean = a.p_emean;
  f.ft_metric = a.ft_metric;
  const ScoreBands sb = score_bands(a.p_fmean, a.p_emean, nc);
  f.p_int = sb.p_int;
  f.p1i = sb.p1i;
  f.p2i = sb.p2i;
  f.m1_lo = sb.m1_lo;
  f.m1_hi = sb.m1_hi;
  f.m2_lo = sb.m2_lo;
  f.m2_hi = sb.m2_hi;
  f.n_obj = a.n_obj;
  for (int o = 0; o < bote::MAXOBJ; ++o) {
    f.obj_kind[o] = a.obj_kind[o];
    f.obj_slot[o] = a.obj_slot[o];
  }
  f.K = s->K;
  f.out_counters = a.out_counters;
  f.want_digest = a.want_digest;
  f.queue = s->queue.as<uint64_t>();
  f.queue_count = s->qcount.as<unsigned long long>();
  f.queue_cap = QUEUE_CAP;
  return BOTE_OK;
}

// Step 3: the fast path.  Decides s->path, fills s->fargs and sizes the fast
// kernel's launch, then plans the group kernel (step 4).  `kernel` forces a
// path (tests, A/B timing; every path is exact); AUTO: the group kernel when
// eligible and >= 90 % lane utilisation.
static int sweep_plan_fast(bote_sweep* s, const uint32_t* servers, const uint32_t* clients, bool fair, int kernel) {
  const bote_planet* p = s->p;
  const EvalArgs& a = s->args;
  const uint32_t n = s->n, ns = s->ns, nc = s->nc, keys = a.keys;
  const bool eligible = fast_eligible(p->lat.data(), p->R, servers, ns, nc, fair) && kernel != BOTE_KERNEL_GENERIC;
  s->path = eligible ? Path::Fast : Path::Generic;
  if (kernel != BOTE_KERNEL_AUTO && kernel != BOTE_KERNEL_GENERIC && !eligible)
    return fail(BOTE_E_ARG, "the fast/group kernel is not eligible for this planet and lists");
  // the extended key set runs on the group kernel (n = 4..7, config 5's
  // objective set, compiled into it, and moments that fit its 32-bit
  // arithmetic: FastLimits::keys32) or on the generic kernel
  const bool compiled_objs = is_compiled_objective_set(a.obj_kind, a.obj_slot, s->n_obj, keys);
  // a MAX objective: the worst-client variant of the fast kernel (base key
  // set), else the generic kernel; a percentile objective: its list variant
  // when every one needs at most PCTL_FAST_DEPTH values, else the generic kernel
  // an MDTM objective: the fast kernel's MDTM variant (base key set), which
  // carries no maxima or lists, so with a MAX or percentile objective beside
  // it the generic kernel
  // (fast_tail_plan, over the key entries: a constrained sweep's constraints
  // count as its objectives do)
  static_assert(TAIL_PLAIN == bote::FAST_PLAIN && TAIL_MAX == bote::FAST_MAX && TAIL_LIST == bote::FAST_LIST &&
                    TAIL_MDTM == bote::FAST_MDTM && DEV_KIND_PCTL == bote::OBJ_PCTL &&
                    DEV_PCTL_NEED_MASK == bote::PCTL_NEED_MASK,
                "the host plan speaks of the kernels' variants and kinds");
  const TailPlan tp = fast_tail_plan(a.obj_kind, (uint32_t)a.n_obj);
  s->tail = tp.tail;
  const uint32_t need = tp.need;
  const bool mdtm_mixed = tp.mixed;
  // a pinned sweep: the fast kernel's pinned variant computes SCORE, MEAN and
  // COV objectives; every other sweep of pinned members runs the generic
  // kernel's pinned variant (launch_sweep_eval)
  if (s->pz.pin_n && s->tail != bote::FAST_PLAIN && s->path != Path::Generic) {
    if (kernel == BOTE_KERNEL_FAST)
      return fail(BOTE_E_ARG, "the fast kernel's pinned variant computes SCORE, MEAN and COV objectives (generic kernel)");
    s->path = Path::Generic;
  }
  const FastLimits lim = fast_limits(p->lat.data(), p->R, nc, n);
  if (keys && eligible &&
      (!bote::group_supports_keys(n, bote::GROUP_XK_MAX_BD) || !compiled_objs || !lim.keys32 ||
       kernel == BOTE_KERNEL_FAST)) {
    if (kernel == BOTE_KERNEL_FAST || kernel == BOTE_KERNEL_GROUP)
      return fail(BOTE_E_ARG, "the extended key set runs on the group kernel (n = 4..7, config 5's "
                              "objectives) or the generic kernel");
    s->path = Path::Generic;
  }
  if (need > (uint32_t)bote::PCTL_FAST_DEPTH && s->path != Path::Generic) {
    if (kernel == BOTE_KERNEL_FAST)
      return fail(BOTE_E_ARG, "the fast kernel's percentile lists are 4 deep: an objective needs " +
                                  std::to_string(need) + " of its slot's largest values (generic kernel)");
    s->path = Path::Generic;
  }
  if (mdtm_mixed && s->path != Path::Generic) {
    if (kernel == BOTE_KERNEL_FAST)
      return fail(BOTE_E_ARG, "the fast kernel's MDTM variant carries no maxima or lists: a sweep with MDTM and MAX or "
                              "percentile objectives runs the generic kernel, which computes both");
    s->path = Path::Generic;
  }
  // a constrained sweep on a variant whose constrained kernel is not built
  if (s->n_con && s->path != Path::Generic && !bote::fast_has_constrained(n, s->tail)) {
    if (kernel == BOTE_KERNEL_FAST)
      return fail(BOTE_E_ARG, "the fast kernel's constrained variant is not built for these kinds (generic kernel)");
    s->path = Path::Generic;
  }
  if (s->path == Path::Generic) return BOTE_OK;
  int rc;
  if ((rc = fill_fast_args(s, servers, clients, lim))) return rc;
  bote::FastArgs& f = s->fargs;
#ifdef BOTE_DEBUG
  if (s->dbg.alloc(16) != hipSuccess || hipMemset(s->dbg.p, 0, 16) != hipSuccess)
    return fail(BOTE_E_NOMEM, "debug flag");
  f.dbg_flag = s->dbg.as<unsigned int>();
#endif
#ifdef BOTE_PATHSTATS
  if (s->pstats.alloc(64 * 8) != hipSuccess || hipMemset(s->pstats.p, 0, 64 * 8) != hipSuccess)
    return fail(BOTE_E_NOMEM, "path counters");
  f.pstats = s->pstats.as<unsigned long long>();
#endif
#ifdef BOTE_ABLATION
  const char* abl = getenv("BOTE_ABLATE");  // timing-diagnostics builds only
  f.ablate = abl ? (uint32_t)strtoul(abl, nullptr, 0) : 0u;
#endif
  s->fshm = bote::fast_smem_bytes(f, n, s->tail);
  if (s->fshm > device_max_lds(p->device)) {
    s->path = Path::Generic;
  } else {
    s->fgrid = (uint32_t)(device_cus(p->device) *
                          bote::fast_occupancy(n, s->tail, s->pz.pin_n != 0, s->fshm, false, s->n_con != 0));
  }
  if ((rc = sweep_plan_group(s, lim, compiled_objs, kernel))) return rc;
  // the fast (non-group) kernel does not compute the extended key set
  if (keys && s->path == Path::Fast) s->path = Path::Generic;
  return BOTE_OK;
}

// Step 5: the per-block lists, the merge buffers, the result block and the
// events.
static int sweep_alloc_workspace(bote_sweep* s) {
  const uint32_t n_obj = s->n_obj;
  // the generic path may also run on a fast sweep (overflow recompute)
  const bool fixup = s->path != Path::Generic;
  const uint32_t lists = fixup ? std::max(s->grid, s->fgrid + s->xgrid) : s->grid;
  size_t top_bytes = (size_t)lists * std::max<uint32_t>(n_obj, 1) * bote::KP * 16;
  size_t tmp_bytes = (size_t)((lists + 7) / 8) * std::max<uint32_t>(n_obj, 1) * bote::KP * 16;
  if (s->top.alloc(top_bytes) != hipSuccess || s->tmp0.alloc(tmp_bytes) != hipSuccess ||
      s->tmp1.alloc(tmp_bytes) != hipSuccess || s->result.alloc(s->result_bytes()) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc sweep workspace");
  if (fixup && (s->top_alt.alloc((size_t)s->grid * std::max<uint32_t>(n_obj, 1) * bote::KP * 16) != hipSuccess ||
                  s->counters_alt.alloc(16) != hipSuccess))
    return fail(BOTE_E_NOMEM, "hipMalloc overflow fallback workspace");
  if (s->n_con && s->admitted.alloc(16) != hipSuccess) return fail(BOTE_E_NOMEM, "hipMalloc admitted counters");
  // (a constrained sweep without objectives still builds its keys: the admitted count)
  s->args.out_top = n_obj || s->n_con ? s->top.as<Rec>() : nullptr;
  s->fargs.out_top = s->args.out_top;
  if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess ||
      hipEventCreateWithFlags(&s->done, hipEventDisableTiming) != hipSuccess)
    return fail(BOTE_E_DEVICE, "hipEventCreate");
  return BOTE_OK;
}

// bote_sweep_create_keys and, with `is_pinned`, bote_sweep_create_pinned
// and, with `cons`, bote_sweep_create_constrained (n_con may be 0)
static int sweep_create(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                        uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                        const bote_ranking_params* rp, int digest, int kernel, uint32_t keys, bool is_pinned,
                        const uint32_t* pinned, uint32_t n_pinned, bote_sweep** out,
                        const bote_constraint* cons = nullptr, uint32_t n_con = 0) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  int rc;
  bool has_score = false;
  if (!out) return fail(BOTE_E_ARG, "out is null");
  ARG_TRY(check_sweep_args(p ? p->R : 0, servers, ns, clients, nc, n, objs, n_obj, K, rp, kernel, keys, has_score));
  if (is_pinned) ARG_TRY(check_pinned_args(ns, n, pinned, n_pinned, kernel, keys));
  ARG_TRY(check_constraint_args(nc, n, cons, n_con, n_obj, kernel, keys));
  HIP_TRY(hipSetDevice(p->device));
  auto* s = new bote_sweep();
  auto cleanup = [&](int code) {
    bote_sweep_destroy(s);
    return code;
  };
  s->p = p;
  s->device = p->device;
  s->n = n;
  s->ns = ns;
  s->nc = nc;
  s->n_obj = n_obj;
  s->K = K;
  if (is_pinned) {
    s->pz.pin_n = n_pinned;
    std::copy(pinned, pinned + n_pinned, s->pz.pin);
    std::sort(s->pz.pin, s->pz.pin + n_pinned);
    s->ptotal = pinned_total(ns, n, n_pinned);
  }
  // the key entries: the objectives, then a constrained sweep's constraints
  std::vector<bote_objective> entries(objs, objs + n_obj);
  s->n_con = n_con;
  s->con.n_lists = n_obj;
  for (uint32_t c = 0; c < n_con; ++c) {
    entries.push_back(bote_objective{cons[c].kind, cons[c].slot});
    s->con.bound[n_obj + c] = cons[c].max_key;
  }
  if ((rc = sweep_upload_lists(s, servers, clients, entries.data(), (uint32_t)entries.size(), rp, has_score, digest,
                               keys)))
    return cleanup(rc);
  const bool fair = has_score && rp && rp->min_fairness_fpaxos_improv != 0.0;
  if ((rc = sweep_plan_fast(s, servers, clients, fair, kernel))) return cleanup(rc);
  if ((rc = sweep_alloc_workspace(s))) return cleanup(rc);
  *out = s;
  return BOTE_OK;
}

int bote_sweep_create_keys(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                           uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj, uint32_t K,
                           const bote_ranking_params* rp, int digest, int kernel, uint32_t keys, bote_sweep** out) {
  return sweep_create(p, servers, ns, clients, nc, n, objs, n_obj, K, rp, digest, kernel, keys, false, nullptr, 0, out);
}

int bote_sweep_create_constrained(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                                  uint32_t nc, uint32_t n, const bote_objective* objs, uint32_t n_obj,
                                  const bote_constraint* cons, uint32_t n_con, uint32_t K,
                                  const bote_ranking_params* rp, int digest, int kernel, bote_sweep** out) {
  return sweep_create(p, servers, ns, clients, nc, n, objs, n_obj, K, rp, digest, kernel, 0, false, nullptr, 0, out,
                      cons, n_con);
}

int bote_sweep_create_pinned(const bote_planet* p, const uint32_t* servers, uint32_t ns, const uint32_t* clients,
                             uint32_t nc, uint32_t n, const uint32_t* pinned, uint32_t n_pinned,
                             const bote_objective* objs, uint32_t n_obj, uint32_t K, const bote_ranking_params* rp,
                             int digest, int kernel, bote_sweep** out) {
  return sweep_create(p, servers, ns, clients, nc, n, objs, n_obj, K, rp, digest, kernel, 0, true, pinned, n_pinned,
                      out);
}

uint64_t bote_pinned_total(uint32_t ns, uint32_t n, uint32_t n_pinned) { return pinned_total(ns, n, n_pinned); }

int bote_pinned_config(uint64_t pinned_rank, uint32_t n, uint32_t ns, const uint32_t* pinned, uint32_t n_pinned,
                       uint32_t* out_positions, uint64_t* out_rank) {
  if (!pinned || !out_positions) return fail(BOTE_E_ARG, "null argument");
  if (n > BOTE_MAX_N) return fail(BOTE_E_RANGE, "config size above 16");
  if (!pinned_config(pinned_rank, n, ns, pinned, n_pinned, out_positions, out_rank))
    return fail(BOTE_E_ARG, "bad pinned list or pinned rank out of range");
  return BOTE_OK;
}

// the rank space of a sweep's launches: C(ns, n), or a pinned sweep's pinned ranks
static Status sweep_rank_span(const bote_sweep* s, uint64_t rank_begin, uint64_t rank_end) {
  return s->pz.pin_n ? check_rank_span_total(s->ptotal, rank_begin, rank_end)
                     : check_rank_span(s->ns, s->n, rank_begin, rank_end);
}

int bote_sweep_is_fast(const bote_sweep* s, int* out) {
  if (!s || !out) return fail(BOTE_E_ARG, "null argument");
  *out = (int)s->path;  // 0 generic, 1 fast, 2 group
  return BOTE_OK;
}

// The cached group walk covering [rb, re) (walked on first use; a handful of
// walks are kept, the oldest dropped first).  Null off the group kernel or
// when the range has too many groups to walk.
static std::shared_ptr<const GroupWalk> walk_for(const bote_sweep* s, uint64_t rb, uint64_t re) {
  if (s->path != Path::Group || re <= rb) return nullptr;
  for (const auto& w : s->walks)
    if (w->covers(rb, re)) return w;
  std::shared_ptr<const GroupWalk> w = walk_groups(s->ns, s->n, s->nc, rb, re);
  if (!w) return nullptr;
  if (s->walks.size() >= 8) s->walks.erase(s->walks.begin());
  s->walks.push_back(w);
  return w;
}

int bote_sweep_split(const bote_sweep* s, uint64_t rank_begin, uint64_t rank_end, uint32_t parts,
                     uint64_t* out_bounds) {
  if (!s || !out_bounds) return fail(BOTE_E_ARG, "null argument");
  if (parts == 0) return fail(BOTE_E_ARG, "parts must be >= 1");
  ARG_TRY(sweep_rank_span(s, rank_begin, rank_end));
  std::vector<uint64_t> b;
  if (rank_end - rank_begin >= (uint64_t)parts * 64) {
    if (auto w = walk_for(s, rank_begin, rank_end)) b = cut_chunks(*w, rank_begin, rank_end, parts);
  }
  if (b.size() != (size_t)parts + 1) {
    b.resize((size_t)parts + 1);
    const uint64_t span = rank_end - rank_begin;
    for (uint32_t i = 0; i <= parts; ++i) b[i] = rank_begin + (uint64_t)(((unsigned __int128)span * i) / parts);
  }
  std::copy(b.begin(), b.end(), out_bounds);
  return BOTE_OK;
}

}  // extern "C"

#ifndef BOTE_CHUNK_TAIL
#define BOTE_CHUNK_TAIL 3  // guided tail rounds of the chunk table (0: equal-cost chunks only)
#endif
// The group kernel's work-chunk table for [rb, re): cut from a cached walk
// and uploaded on `st` once per range (a bench or a shard re-launches the same
// range).  Null chunks (even rank split in the kernel) off the group kernel.
int bote::capi::sweep_chunks(bote_sweep* s, uint64_t rb, uint64_t re, hipStream_t st, const Chunks** out) {
  *out = nullptr;
  if (s->path != Path::Group) return BOTE_OK;
  HIP_TRY(s->chunks.lookup(rb, re, s->last_stream, st, *out));
  if (!*out) {
    auto c = std::make_unique<Chunks>();
    const uint32_t nwaves = s->fgrid * (s->fargs.gbd / 64);
    // (no chunk below ~4 wavefront steps of configs)
    const char* cpw_env = getenv("BOTE_CHUNKS_PER_WAVE");  // (A/B timing)
    const uint64_t cpw = cpw_env ? std::max(1ul, strtoul(cpw_env, nullptr, 0))
                                 : (uint64_t)chunks_per_wave(re - rb, nwaves, s->fargs.nc, BOTE_CHUNKS_PER_WAVE);
    const uint64_t want = std::min<uint64_t>((uint64_t)nwaves * cpw, (re - rb) / 256 + 1);
    // guided: the launch's last chunks shrink (BOTE_CHUNK_TAIL rounds of one
    // chunk per wave at 1/2, 1/4, ... of the base size), so the waves finish
    // within a small chunk of each other instead of a base chunk
    if (auto w = walk_for(s, rb, re)) c->host = cut_chunks_guided(*w, rb, re, (uint32_t)want, nwaves, BOTE_CHUNK_TAIL);
    if (!c->host.empty()) {
      c->n = (uint32_t)c->host.size() - 1;
      if (c->dev.alloc(c->host.size() * 8) != hipSuccess) return fail(BOTE_E_NOMEM, "hipMalloc work chunks");
      HIP_TRY(hipMemcpyAsync(c->dev.p, c->host.data(), c->host.size() * 8, hipMemcpyHostToDevice, st));
      // each chunk's first group (FastArgs::wstate): the kernel starts a
      // chunk with two loads instead of a device unrank
      if (!chunk_states(c->host.data(), c->n, s->n, s->ns, c->state)) return fail(BOTE_E_ARG, "chunk rank out of range");
      if (c->sdev.alloc(c->state.size() * 8) != hipSuccess) return fail(BOTE_E_NOMEM, "hipMalloc chunk states");
      HIP_TRY(hipMemcpyAsync(c->sdev.p, c->state.data(), c->state.size() * 8, hipMemcpyHostToDevice, st));
    }
    *out = s->chunks.insert(rb, re, std::move(c));
  }
  return BOTE_OK;
}

void bote::capi::unpack_result(const bote_sweep* s, const std::vector<uint8_t>& blk, bote_topk_record* out,
                               uint32_t* out_count, uint64_t* out_valid, uint64_t* out_digest) {
  static_assert(sizeof(bote_topk_record) == sizeof(TopkRecord), "record layout");
  bote::host::unpack_result(blk.data(), s->n_obj, s->K, bote::KP, (TopkRecord*)out, out_count, out_valid, out_digest);
}

// Merge `lists` lists of `src` (list i of objective o at src[i * lstride + o *
// KP]) into the result block (n_obj x KP records, then the two counters at
// record lstride): one launch when the group kernel bounded its lists (kbound:
// few records per list), else the tree of 8-way merges (full lists) through
// tmp0 / tmp1 (ceil(max(lists, alt_lists) / 8) lists each).
// With `sel` (fast path), the first level reads the overflow fallback's
// `alt_lists` lists and counters instead when *sel > cap (on the device).
static bool wide_merge(uint32_t lists, uint32_t alt_lists) {
  return lists <= bote::WIDE_MERGE_LISTS && alt_lists <= bote::WIDE_MERGE_LISTS;
}
int bote::capi::merge_lists(const Rec* src, uint32_t lists, const Rec* alt, uint32_t alt_lists, uint64_t lstride,
                            const unsigned long long* sel, uint64_t cap, const unsigned long long* kbound, Rec* tmp0,
                            Rec* tmp1, void* result, uint32_t n_obj, uint32_t K, const unsigned long long* counters,
                            const unsigned long long* counters_alt, hipStream_t st) {
  Rec* rec_out = (Rec*)result;
  uint64_t* cdst = (uint64_t*)((char*)result + lstride * 16);
  if (n_obj && kbound && sel && wide_merge(lists, alt_lists)) {
    // one launch: the lists' filled prefixes gathered and ranked in LDS, and
    // the counters picked by the same device choice
    HIP_TRY(bote::launch_merge_wide(src, lists, alt, alt_lists, lstride, sel, cap, kbound, rec_out, n_obj, K, counters,
                                    counters_alt, cdst, st));
    return BOTE_OK;
  }
  if (n_obj) {
    Rec* bufs[2] = {tmp0, tmp1};
    int b = 0;
    if (sel) {
      Rec* dst = lists > bote::G_MERGE_LISTS || alt_lists > bote::G_MERGE_LISTS ? bufs[b] : rec_out;
      HIP_TRY(bote::launch_merge(src, lists, alt, alt_lists, lstride, sel, cap, dst, lstride, n_obj, st));
      lists = (std::max(lists, alt_lists) + bote::G_MERGE_LISTS - 1) / bote::G_MERGE_LISTS;
      src = dst;
      b ^= 1;
      if (dst == rec_out) lists = 0;
    }
    while (lists > bote::G_MERGE_LISTS) {
      HIP_TRY(bote::launch_merge(src, lists, nullptr, 0, lstride, nullptr, 0, bufs[b], lstride, n_obj, st));
      src = bufs[b];
      b ^= 1;
      lists = (lists + bote::G_MERGE_LISTS - 1) / bote::G_MERGE_LISTS;
    }
    if (lists) HIP_TRY(bote::launch_merge(src, lists, nullptr, 0, lstride, nullptr, 0, rec_out, lstride, n_obj, st));
  }
  if (sel) {
    HIP_TRY(bote::launch_pick_counters(counters, counters_alt, sel, cap, cdst, st));
  } else {
    HIP_TRY(hipMemcpyAsync(cdst, counters, 16, hipMemcpyDeviceToDevice, st));
  }
  return BOTE_OK;
}

extern "C" {

// Merge `lists` per-block lists into the result block and append the counters
// (merge_lists on the sweep's buffers).
static int merge_chain(bote_sweep* s, uint32_t lists, hipStream_t st, const unsigned long long* sel = nullptr,
                       uint32_t alt_lists = 0, const unsigned long long* kbound = nullptr) {
  return merge_lists(s->top.as<Rec>(), lists, s->top_alt.as<Rec>(), alt_lists, (uint64_t)s->n_obj * bote::KP, sel,
                     QUEUE_CAP, kbound, s->tmp0.as<Rec>(), s->tmp1.as<Rec>(), s->result.p, s->n_obj, s->K,
                     s->counters.as<unsigned long long>(), s->counters_alt.as<unsigned long long>(), st);
}

static int timing_slot(bote_sweep* s, hipEvent_t*& e0, hipEvent_t*& e1) {
  if (s->ev_used == s->evpool.size()) {
    hipEvent_t a0, a1;
    HIP_TRY(hipEventCreate(&a0));
    HIP_TRY(hipEventCreate(&a1));
    s->evpool.emplace_back(a0, a1);
  }
  auto& tp = s->evpool[s->ev_used++];
  e0 = &tp.first;
  e1 = &tp.second;
  return BOTE_OK;
}

// a constrained sweep's ConArgs with the counter s->admitted[adm]
static bote::ConArgs con_args(const bote_sweep* s, int adm) {
  bote::ConArgs z = s->con;
  z.admitted = s->admitted.as<unsigned long long>() + adm;
  return z;
}

// The generic kernel's top-K launch with `a` on the sweep's grid (a pinned
// sweep: its pinned variant, [a.rb, a.re) being pinned ranks)
// (a constrained sweep: its constrained variant, counting into s->admitted[adm])
static hipError_t launch_sweep_eval(const bote_sweep* s, const EvalArgs& a, hipStream_t st, int adm = 0) {
  if (s->n_con) return bote::launch_eval_con(a, s->n, con_args(s, adm), s->grid, s->bd, s->shm, st);
  return bote::launch_eval(a, s->n, false, s->grid, s->bd, s->shm, st, s->pz.pin_n ? &s->pz : nullptr);
}

// Generic kernel over [rb, re): the exact path for any planet.
static int launch_generic(bote_sweep* s, uint64_t rb, uint64_t re, hipStream_t st, bool timed) {
  EvalArgs a = s->args;
  a.rb = rb;
  a.re = re;
  a.runlen = sweep_runlen(re - rb, s->grid, s->bd);
  HIP_TRY(hipMemsetAsync(s->counters.p, 0, 16, st));
  if (s->n_con) HIP_TRY(hipMemsetAsync(s->admitted.p, 0, 16, st));
  hipEvent_t *e0 = nullptr, *e1 = nullptr;
  int rc;
  if (timed && (rc = timing_slot(s, e0, e1))) return rc;
  s->last0 = e0 ? *e0 : s->ev0;
  s->last1 = e1 ? *e1 : s->ev1;
  HIP_TRY(hipEventRecord(s->last0, st));
  HIP_TRY(launch_sweep_eval(s, a, st));
  HIP_TRY(hipEventRecord(s->last1, st));
  return merge_chain(s, s->grid, st);
}

// The top-K seed of a group launch over [rb, re) (launch_fast_path): sets
// f.tseed, or leaves it null when the range is too small to sample.
// The sample plan (how many one-step chunks, where) is bote_host.cpp's
// sample_count / sample_starts.
static int sample_seed(bote_sweep* s, bote::FastArgs& f, uint64_t rb, uint64_t re, hipStream_t st) {
  const uint32_t nwaves = s->fgrid * (s->fargs.gbd / 64);
  const uint32_t nsamp = sample_count(rb, re, binom_u64(s->ns, s->n), nwaves, s->K);
  if (!nsamp) return BOTE_OK;
  const Chunks* c = nullptr;
  HIP_TRY(s->samples.lookup(rb, re, s->last_stream, st, c));
  if (!c) {
    auto t = std::make_unique<Chunks>();
    t->n = nsamp;
    t->host = sample_starts(rb, re, nsamp);
    if (!chunk_states(t->host.data(), nsamp, s->n, s->ns, t->state)) return fail(BOTE_E_ARG, "sample rank out of range");
    if (t->dev.alloc(t->host.size() * 8) != hipSuccess || t->sdev.alloc(t->state.size() * 8) != hipSuccess)
      return fail(BOTE_E_NOMEM, "hipMalloc sample chunks");
    HIP_TRY(hipMemcpyAsync(t->dev.p, t->host.data(), t->host.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(t->sdev.p, t->state.data(), t->state.size() * 8, hipMemcpyHostToDevice, st));
    c = s->samples.insert(rb, re, std::move(t));
  }
  // slots: one per wave (K slots at or below a key are K distinct configs: the
  // waves' chunks are disjoint), or one per chunk on grids of fewer than K waves
  const uint32_t slots = nwaves >= s->K ? nwaves : nsamp;
  if (s->smin.reserve((size_t)s->n_obj * slots * 8) != hipSuccess || s->tseed.reserve(bote::MAXOBJ * 8) != hipSuccess)
    return fail(BOTE_E_NOMEM, "hipMalloc top-K seed");
  // (per-wave slots: each wave clears its own at the sample launch's start)
  if (slots != nwaves || slots == nsamp) HIP_TRY(hipMemsetAsync(s->smin.p, 0xFF, (size_t)s->n_obj * slots * 8, st));
  bote::FastArgs fs = f;
  fs.smin = s->smin.as<uint64_t>();
  fs.tseed = nullptr;
  fs.wchunks = c->dev.as<uint64_t>();
  fs.wstate = c->sdev.as<uint64_t>();
  fs.nwchunks = nsamp;
  fs.ssteps = 1;  // one step per sample chunk (one group precompute each)
  fs.smin_wave = slots == nwaves && slots != nsamp ? 1u : 0u;
  fs.wctr = f.wctr + 256;  // the sample launch's ticket shards
  HIP_TRY(bote::launch_group(fs, s->n, s->def_obj, s->fgrid, s->fshm, st));
  HIP_TRY(bote::launch_seed(fs.smin, fs.smin_wave ? nwaves : nsamp, s->n_obj, s->K, s->tseed.as<uint64_t>(), st));
  f.tseed = s->tseed.as<uint64_t>();
  return BOTE_OK;
}

// Fast kernel over [rb, re), then the generic kernel over its deferred ranks.
static int launch_fast_path(bote_sweep* s, uint64_t rb, uint64_t re, hipStream_t st) {
  bote::FastArgs f = s->fargs;
  f.rb = rb;
  f.re = re;
  f.runlen = sweep_runlen(re - rb, s->fgrid, bote::FAST_BD);
  const bool group = s->path == Path::Group;
  if (group) {
    // cost-balanced chunks (32 per wave), taken dynamically (bote_group.hip)
    const Chunks* ch = nullptr;
    int crc = sweep_chunks(s, rb, re, st, &ch);
    if (crc) return crc;
    f.nwchunks = ch ? ch->n : 0;
    f.wchunks = ch ? ch->dev.as<uint64_t>() : nullptr;
    f.wstate = ch && !ch->state.empty() ? ch->sdev.as<uint64_t>() : nullptr;
    if (f.nwchunks) {
      // (8 shards of 128 B for the main launch, 8 for the sample launch)
      if (!s->wctr.p && s->wctr.alloc(16 * 128) != hipSuccess) return fail(BOTE_E_NOMEM, "hipMalloc work counters");
      f.wctr = s->wctr.as<unsigned int>();
      // 8 counter shards when the grid divides evenly (equal blocks per shard)
      f.wshards = s->fgrid % 8 == 0 ? 8u : 1u;
    }
  }
  // counters, deferred count, work tickets, fallback counters: one launch
  // the group blocks' lists shrink to the records within the least K-th key
  // of any block's list when the one-launch merge reads them
  f.kbound = nullptr;
  if (group && s->n_obj && s->K && wide_merge(s->fgrid + s->xgrid, s->grid)) {
    if (!s->kbound.p && s->kbound.alloc(bote::MAXOBJ * 8) != hipSuccess) return fail(BOTE_E_NOMEM, "hipMalloc K-th key bound");
    f.kbound = s->kbound.as<unsigned long long>();
  }
  HIP_TRY(bote::launch_zero_ctl(s->counters.as<unsigned long long>(), s->qcount.as<unsigned long long>(),
                                f.nwchunks ? f.wctr : nullptr, s->counters_alt.as<unsigned long long>(), f.kbound, st));
  if (s->n_con) HIP_TRY(hipMemsetAsync(s->admitted.p, 0, 16, st));
  // top-K seed: one step of 64 configs per wave at evenly spaced ranks, then
  // per objective the K-th least of the chunks' minimum keys (a bound on the
  // range's K-th key: K distinct configs of the range reach it), so that the
  // blocks' lists start with a threshold instead of filling from empty (the
  // fill costs about the same per block whatever the range: at 1/8 of R=64
  // n=7 it was 1/8 of the kernel)
  if (group && f.nwchunks && s->n_obj && s->K) {
    int src = sample_seed(s, f, rb, re, st);
    if (src) return src;
  }
  hipEvent_t *e0 = nullptr, *e1 = nullptr;
  int rc;
  if ((rc = timing_slot(s, e0, e1))) return rc;
  // the kernel's events ride on its dispatch (hipExtLaunchKernel): a
  // separate hipEventRecord before and after the kernel left ~10 us of idle
  // GPU each (profiles/r05b trace)
  s->last0 = *e0;
  s->last1 = *e1;
  if (group) HIP_TRY(bote::launch_group(f, s->n, s->def_obj, s->fgrid, s->fshm, st, *e0, *e1));
  else if (s->n_con) HIP_TRY(bote::launch_fast_con(f, s->n, s->tail, con_args(s, 0), s->fgrid, s->fshm, st, *e0, *e1));
  else HIP_TRY(bote::launch_fast(f, s->n, s->tail, s->pz.pin_n ? &s->pz : nullptr, s->fgrid, s->fshm, st, *e0, *e1));
  // exact fixup of the deferred configs: generic kernel over the rank list
  EvalArgs a = s->args;
  a.rank_list = s->queue.as<uint64_t>();
  a.rank_count = s->qcount.as<unsigned long long>();
  a.rb = 0;
  a.re = QUEUE_CAP;
  a.runlen = 1;
  a.out_top = s->n_obj || s->n_con ? s->top.as<Rec>() + (size_t)s->fgrid * s->n_obj * bote::KP : nullptr;
  // (a constrained sweep: the deferred configs are admitted or rejected here, and counted with the fast kernel's)
  if (s->n_con) HIP_TRY(bote::launch_eval_con(a, s->n, con_args(s, 0), s->xgrid, s->bd, s->shm, st));
  else HIP_TRY(bote::launch_eval(a, s->n, false, s->xgrid, s->bd, s->shm, st));
  // overflow fallback: more deferred configs than the queue holds => the
  // generic kernel recomputes the whole range into its own lists/counters and
  // the merge picks those.  Decided on the device (every block of the fallback
  // exits at once otherwise): no host round trip per launch.
  EvalArgs g = s->args;
  g.rb = rb;
  g.re = re;
  g.runlen = sweep_runlen(re - rb, s->grid, s->bd);
  g.out_top = s->n_obj || s->n_con ? s->top_alt.as<Rec>() : nullptr;
  g.out_counters = s->counters_alt.as<unsigned long long>();
  g.run_if_over = s->qcount.as<unsigned long long>();
  g.over_cap = QUEUE_CAP;
  // (a constrained sweep: the fallback counts the whole range into a counter
  // of its own, which bote_sweep_admitted reads in place of the first)
  HIP_TRY(launch_sweep_eval(s, g, st, 1));
  return merge_chain(s, s->fgrid + s->xgrid, st, s->qcount.as<unsigned long long>(), s->grid, f.kbound);
}

int bote_sweep_launch(bote_sweep* s, uint64_t rank_begin, uint64_t rank_end, void* hip_stream) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s) return fail(BOTE_E_ARG, "sweep is null");
  ARG_TRY(sweep_rank_span(s, rank_begin, rank_end));
  HIP_TRY(hipSetDevice(s->p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  int rc = s->path == Path::Generic ? launch_generic(s, rank_begin, rank_end, st, true)
                                    : launch_fast_path(s, rank_begin, rank_end, st);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->done, st));
  s->last_rb = rank_begin;
  s->last_re = rank_end;
  s->last_stream = st;
  s->launched = true;
  return BOTE_OK;
}

uint64_t bote_sweep_result_bytes(const bote_sweep* s) { return s ? s->result_bytes() : 0; }

#ifdef BOTE_PATHSTATS
// Path-statistics builds only (not in include/bote_hip.h): the 64 group-kernel
// path counters since the last call (read, then reset; scripts/pathstats.py).
int bote_sweep_pathstats(bote_sweep* s, uint64_t* out) {
  DevGuard dev_guard;
  if (!s || !out || !s->pstats.p) return fail(BOTE_E_ARG, "no path counters");
  HIP_TRY(hipSetDevice(s->p->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out, s->pstats.p, 64 * 8, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemset(s->pstats.p, 0, 64 * 8));
  return BOTE_OK;
}
#endif

int bote_sweep_result_device(bote_sweep* s, void* dst, void* hip_stream) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !dst) return fail(BOTE_E_ARG, "null argument");
  if (!s->launched) return fail(BOTE_E_ARG, "sweep not launched");
  HIP_TRY(hipSetDevice(s->p->device));
  // (dst: device memory, or pinned host memory: the direct device-to-host copy)
  HIP_TRY(hipMemcpyAsync(dst, s->result.p, s->result_bytes(), hipMemcpyDefault, (hipStream_t)hip_stream));
  HIP_TRY(hipEventRecord(s->done, (hipStream_t)hip_stream));
  return BOTE_OK;
}

int bote_sweep_result(bote_sweep* s, void* hip_stream, bote_topk_record* out, uint32_t* out_count,
                      uint64_t* out_valid, uint64_t* out_digest) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s) return fail(BOTE_E_ARG, "sweep is null");
  if (!s->launched) return fail(BOTE_E_ARG, "sweep not launched");
  HIP_TRY(hipSetDevice(s->p->device));
  std::vector<uint8_t> blk(s->result_bytes());
  HIP_TRY(hipMemcpyAsync(blk.data(), s->result.p, blk.size(), hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
#ifdef BOTE_DEBUG
  if (s->dbg.p) {
    unsigned int flag = 0;
    HIP_TRY(hipMemcpy(&flag, s->dbg.p, 4, hipMemcpyDeviceToHost));
    if (flag) return fail(BOTE_E_DEVICE, "device assert failed (BOTE_DEBUG), flag bits " + std::to_string(flag));
  }
#endif
  unpack_result(s, blk, out, out_count, out_valid, out_digest);
  return BOTE_OK;
}

int bote_merge_device(const bote_sweep* s, const void* src, uint32_t n_shards, void* dst, void* hip_stream) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !src || !dst || n_shards == 0) return fail(BOTE_E_ARG, "bad merge arguments");
  if (n_shards > bote::G_MERGE_LISTS) return fail(BOTE_E_RANGE, "at most 8 shards per merge call");
  HIP_TRY(hipSetDevice(s->p->device));
  hipStream_t st = (hipStream_t)hip_stream;
  const uint64_t bstride = s->result_bytes() / 16;  // records per block
  const uint64_t lstride = (uint64_t)s->n_obj * bote::KP;
  if (s->n_obj)
    HIP_TRY(bote::launch_merge((const Rec*)src, n_shards, nullptr, 0, bstride, nullptr, 0, (Rec*)dst, lstride, s->n_obj, st));
  HIP_TRY(bote::launch_sum_counters((const uint64_t*)src, n_shards, bstride * 2, lstride * 2,
                                    (uint64_t*)dst + lstride * 2, st));
  return BOTE_OK;
}

int bote_sweep_last_kernel_ms(bote_sweep* s, float* out_ms) {
  if (!s || !out_ms) return fail(BOTE_E_ARG, "null argument");
  if (!s->launched) return fail(BOTE_E_ARG, "sweep not launched");
  HIP_TRY(hipEventSynchronize(s->last1));
  HIP_TRY(hipEventElapsedTime(out_ms, s->last0, s->last1));
  return BOTE_OK;
}

int bote_sweep_timing_reset(bote_sweep* s) {
  if (!s) return fail(BOTE_E_ARG, "sweep is null");
  s->ev_used = 0;
  return BOTE_OK;
}

int bote_sweep_timing(bote_sweep* s, float* out_total_ms, uint32_t* out_launches) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !out_total_ms || !out_launches) return fail(BOTE_E_ARG, "null argument");
  HIP_TRY(hipSetDevice(s->p->device));
  float tot = 0.f;
  for (size_t i = 0; i < s->ev_used; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventSynchronize(s->evpool[i].second));
    HIP_TRY(hipEventElapsedTime(&ms, s->evpool[i].first, s->evpool[i].second));
    tot += ms;
  }
  *out_total_ms = tot;
  *out_launches = (uint32_t)s->ev_used;
  return BOTE_OK;
}

int bote_sweep_deferred(bote_sweep* s, void* hip_stream, uint64_t* out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !out) return fail(BOTE_E_ARG, "null argument");
  *out = 0;
  if (s->path == Path::Generic || !s->launched) return BOTE_OK;
  HIP_TRY(hipSetDevice(s->p->device));
  unsigned long long q = 0;
  HIP_TRY(hipMemcpyAsync(&q, s->qcount.p, 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  *out = q;
  return BOTE_OK;
}

int bote_sweep_admitted(bote_sweep* s, void* hip_stream, uint64_t* out) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s || !out) return fail(BOTE_E_ARG, "null argument");
  *out = 0;
  if (!s->launched) return fail(BOTE_E_ARG, "sweep not launched");
  if (!s->n_con) {
    *out = s->last_re - s->last_rb;
    return BOTE_OK;
  }
  HIP_TRY(hipSetDevice(s->p->device));
  unsigned long long q = 0, adm[2] = {0, 0};
  if (s->path != Path::Generic)
    HIP_TRY(hipMemcpyAsync(&q, s->qcount.p, 8, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipMemcpyAsync(adm, s->admitted.p, 16, hipMemcpyDeviceToHost, (hipStream_t)hip_stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)hip_stream));
  *out = q > QUEUE_CAP ? adm[1] : adm[0];  // (the merge's own choice of the fallback's lists)
  return BOTE_OK;
}

int bote_sweep_grid(const bote_sweep* s, uint32_t* out_grid, uint32_t* out_block, uint32_t* out_lds_bytes) {
  if (!s) return fail(BOTE_E_ARG, "sweep is null");
  const bool generic = s->path == Path::Generic;
  if (out_grid) *out_grid = generic ? s->grid : s->fgrid;
  if (out_block) *out_block = generic ? s->bd : s->path == Path::Group ? s->fargs.gbd : bote::FAST_BD;
  if (out_lds_bytes) *out_lds_bytes = (uint32_t)(generic ? s->shm : s->fshm);
  return BOTE_OK;
}

int bote_sweep_destroy(bote_sweep* s) {
  DevGuard dev_guard;  // the caller's current device is restored on return
  if (!s) return BOTE_OK;
  (void)hipSetDevice(s->device);  // (not s->p->device: the planet may have been destroyed first)
  // work the last launch or result copy enqueued may still run (a launch
  // without a result call): wait for it before the buffers are freed and
  // handed to the next allocation.  An event, not the caller's stream (it may
  // be gone by now) and not the device (hipDeviceSynchronize would also wait
  // for other sweeps' and other threads' work: ADVICE r05)
  if (s->done) {
    if (s->launched) (void)hipEventSynchronize(s->done);
    (void)hipEventDestroy(s->done);
  }
  for (auto& e : s->evpool) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  if (s->ev0) (void)hipEventDestroy(s->ev0);
  if (s->ev1) (void)hipEventDestroy(s->ev1);
  delete s;
  return BOTE_OK;
}

}  // extern "C"
