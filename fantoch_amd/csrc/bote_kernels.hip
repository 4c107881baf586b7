// bote_kernels.hip — the generic exact kernel's launchers (eval_kernel itself
// is the template of bote_eval.hpp, instantiated by family in the
// bote_eval_*.hip units; eval_fn here picks among them) and the
// single-configuration kernels of the per-call Bote::* API.  The top-K lists'
// merge, seed and counters are in bote_merge.hip.
//
// Reference map (eval_kernel's is in bote_eval.hpp):
//   k_single_*             Bote::{leaderless, leader, all_leaders_stats, best_leader}
#include "bote_eval.hpp"
#include "bote_launch.hpp"

namespace bote {

// ------------------------------------------------- single-config kernels --
// Shared by Bote::{leaderless, leader, all_leaders_stats, best_leader}.
// Server membership is a set (the reference filters with `contains`).


// q-th closest (1-based) from row `from` over the member set: counting
// selection, O(R) per call over the set members in (latency, id) order.
__device__ inline uint32_t quorum_lat(const uint32_t* smat, const uint8_t* member, uint32_t R, uint32_t from, uint32_t q,
                                      int* err) {
  // the q-th smallest of { L[from][t] : member[t] } (ties irrelevant for the value)
  for (uint32_t t = 0; t < R; ++t) {
    if (!member[t]) continue;
    uint32_t v = smat[from * R + t] >> LAT_SHIFT;
    uint32_t lt = 0, le = 0;
    for (uint32_t u = 0; u < R; ++u) {
      if (!member[u]) continue;
      uint32_t w = smat[from * R + u] >> LAT_SHIFT;
      lt += w < v;
      le += w <= v;
    }
    if (lt < q && q <= le) return v;
  }
  if (err) *err = 1;
  return 0;
}

__device__ inline uint32_t closest_member(const uint32_t* smat, const uint8_t* member, uint32_t R, uint32_t from) {
  // packed (latency << 8 | id) min: the (latency, name) order with id == name rank
  uint32_t key = 0xFFFFFFFFu;
  for (uint32_t t = 0; t < R; ++t)
    if (member[t]) key = min(key, ((smat[from * R + t] >> LAT_SHIFT) << 8) | t);
  return key;
}

// mode 0: quorum latencies of `froms`; 1: leaderless; 2: leader; 3: all leaders
__global__ void __launch_bounds__(256) single_kernel(SingleArgs a, int mode) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t* smat = (uint32_t*)smem;
  uint8_t* member = (uint8_t*)(smat + a.R * a.R);
  uint32_t* qlat = (uint32_t*)(smem + align_up(a.R * a.R * 4 + a.R, 16));
  for (uint32_t i = threadIdx.x; i < a.R * a.R; i += blockDim.x) smat[i] = a.mat[i];
  for (uint32_t i = threadIdx.x; i < a.R; i += blockDim.x) member[i] = 0;
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < a.ns; i += blockDim.x) member[a.servers[i]] = 1;
  __syncthreads();
  // quorum latency of every region (only member rows are used)
  for (uint32_t r = threadIdx.x; r < a.R; r += blockDim.x) qlat[r] = quorum_lat(smat, member, a.R, r, a.q, a.err);
  __syncthreads();
  if (mode == 0) {
    for (uint32_t i = threadIdx.x; i < a.nf; i += blockDim.x) a.out[i] = qlat[a.froms[i]];
  } else if (mode == 1) {
    for (uint32_t i = threadIdx.x; i < a.nc; i += blockDim.x) {
      uint32_t c = a.clients[i];
      uint32_t key = closest_member(smat, member, a.R, c);
      a.out[i] = (uint64_t)(key >> 8) + qlat[key & 0xFF];
    }
  } else if (mode == 2) {
    for (uint32_t i = threadIdx.x; i < a.nc; i += blockDim.x) {
      uint32_t c = a.clients[i];
      a.out[i] = (uint64_t)(smat[c * a.R + a.leader] >> LAT_SHIFT) + qlat[a.leader];
    }
  } else {
    for (uint32_t i = threadIdx.x; i < a.ns * a.nc; i += blockDim.x) {
      uint32_t l = a.servers[i / a.nc], c = a.clients[i % a.nc];
      a.out[i] = (uint64_t)(smat[c * a.R + l] >> LAT_SHIFT) + qlat[l];
    }
  }
}

// Bote::best_leader: one thread per leader computes the reference's f64 stat
// (ordered sums), then thread 0 takes the first minimum under F64's order.
__global__ void __launch_bounds__(256) best_leader_kernel(SingleArgs a, const uint64_t* vals, double* stat) {
  for (uint32_t l = threadIdx.x; l < a.ns; l += blockDim.x) {
    const uint64_t* v = vals + (size_t)l * a.nc;
    uint64_t s1 = 0;
    for (uint32_t c = 0; c < a.nc; ++c) s1 += v[c];
    auto gen = [&](uint32_t c) { return (uint32_t)v[c]; };
    double x;
    if (a.stat == 0) x = (double)s1 / (double)a.nc;
    else if (a.stat == 1) x = ref_cov(gen, a.nc, s1);
    else x = ref_mdtm(gen, a.nc, s1);
    stat[l] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t b = 0;
    for (uint32_t l = 1; l < a.ns; ++l)
      if (f64_cmp(stat[l], stat[b]) < 0) b = l;
    *a.out_pos = b;
  }
}

// ------------------------------------------------------------- launchers --
size_t eval_smem_bytes(const EvalArgs& a, uint32_t n, uint32_t bd, bool topk) {
  size_t off[12];
  int nl = 0;
  const bool x = a.keys != 0;
  switch (n) {
#define NL_CASE(NN) case NN: nl = x ? QTab<NN, true>::NT : QTab<NN, false>::NT; break;
    BOTE_EVAL_SIZES(NL_CASE)
#undef NL_CASE
    default: return 0;
  }
  return smem_layout(a, (int)n, (nl + 1) / 2, bd, topk, off);
}

// the kernel for config size n, full outputs or top-K, base or extended keys
// (null: unsupported), for the occupancy query and the launch alike: the one
// map from (n, full, keys, passes, pin) to a family's lookup (bote_eval.hpp)
// `passes` (EVAL_*): the top-K instantiation that also computes percentile
// objectives, or those and MDTM objectives
// `pin`: the pinned variant (bote_pinned.hpp; top-K, base keys): EVAL_PLAIN, or
// EVAL_MDTM for a sweep with a percentile or an MDTM objective (each level has
// the passes of the ones below it)
// `census`: the census variant (bote_census.hpp; base keys, unpinned): EVAL_PLAIN,
// or EVAL_MDTM for a census with a MAX, percentile or MDTM objective
// `con`: the constrained variant (base keys, unpinned, top-K): the same two
static const void* eval_fn(uint32_t n, bool full, bool keys, int passes, bool pin, bool census = false,
                           bool con = false) {
  if (con) return full || keys || pin || census ? nullptr : eval_fn_con(n, passes != EVAL_PLAIN);
  if (census) return full || keys || pin ? nullptr : eval_fn_census(n, passes != EVAL_PLAIN);
  if (pin) return full || keys ? nullptr : eval_fn_pinned(n, passes != EVAL_PLAIN);
  if (full) return eval_fn_full(n, keys);
  if (passes >= EVAL_MDTM) return eval_fn_mdtm(n, keys);
  if (passes == EVAL_PCTL) return eval_fn_pctl(n, keys);
  return eval_fn_topk(n, keys);
}

int eval_occupancy(uint32_t n, bool full, uint32_t bd, size_t shm, bool keys, int passes, bool pin, bool census,
                   bool con) {
  const void* k = eval_fn(n, full, keys, passes, pin, census, con);
  return k ? kernel_occupancy(k, bd, shm, 1) : 0;
}

hipError_t launch_eval(const EvalArgs& a, uint32_t n, bool full, uint32_t grid, uint32_t bd, size_t shm,
                       hipStream_t st, const PinArgs* pin) {
  // a percentile or MDTM objective among a top-K sweep's (bote_kernels.hpp EVAL_*)
  const int passes = full ? (int)EVAL_PLAIN : eval_passes(a.obj_kind, a.n_obj);
  const void* k = eval_fn(n, full, a.keys != 0, passes, pin != nullptr);
  if (!k) return hipErrorInvalidValue;
  if (!pin) return launch_kernel(k, a, grid, bd, shm, st);
  PinEvalArgs pa{};
  static_cast<EvalArgs&>(pa) = a;
  pa.pz = *pin;
  return launch_kernel(k, pa, grid, bd, shm, st);
}

hipError_t launch_eval_con(const EvalArgs& a, uint32_t n, const ConArgs& z, uint32_t grid, uint32_t bd, size_t shm,
                           hipStream_t st) {
  const void* k = eval_fn(n, false, a.keys != 0, eval_passes(a.obj_kind, a.n_obj), false, false, true);
  if (!k || a.cfgs || !z.admitted || a.n_obj > MAXOBJ || z.n_lists > (uint32_t)a.n_obj) return hipErrorInvalidValue;
  ConEvalArgs ca{};
  static_cast<EvalArgs&>(ca) = a;
  ca.cz = z;
  return launch_kernel(k, ca, grid, bd, shm, st);
}

hipError_t launch_eval_census(const EvalArgs& a, uint32_t n, const CensusArgs& z, uint32_t grid, uint32_t bd,
                              size_t shm, hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const void* k = eval_fn(n, false, a.keys != 0, eval_passes(a.obj_kind, a.n_obj), false, true);
  if (!k || a.cfgs || !z.thr || !z.below || z.T == 0 || z.T > (uint32_t)CENSUS_T || bd != 256)
    return hipErrorInvalidValue;
  CensusEvalArgs ca{};
  static_cast<EvalArgs&>(ca) = a;
  ca.out_top = nullptr;
  ca.cz = z;
  return launch_kernel(k, ca, grid, bd, shm, st, e0, e1);
}

hipError_t launch_single(const SingleArgs& a, int mode, hipStream_t st) {
  size_t shm = align_up((size_t)a.R * a.R * 4 + a.R, 16) + (size_t)a.R * 4;
  hipError_t e = hipFuncSetAttribute((const void*)single_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(single_kernel, dim3(1), dim3(256), shm, st, a, mode);
  return hipGetLastError();
}

hipError_t launch_best_leader(const SingleArgs& a, const uint64_t* vals, double* stat, hipStream_t st) {
  hipLaunchKernelGGL(best_leader_kernel, dim3(1), dim3(256), 0, st, a, vals, stat);
  return hipGetLastError();
}

}  // namespace bote
