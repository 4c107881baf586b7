// bote_kernels.hip — the generic exact kernel (eval_kernel: any planet,
// explicit configs or colex ranks, full outputs or block top-K lists) and the
// single-configuration kernels of the per-call Bote::* API.  The top-K lists'
// merge, seed and counters are in bote_merge.hip.
//
// Work mapping (DESIGN.md "Kernels"): one LANE evaluates one configuration at a
// time; a wavefront holds 64 neighbouring configurations (colex-consecutive
// ranks), so every per-client step is wave-uniform in the client and
// lane-varying only in the config's members.  The R x R latency matrix (stored
// latency << 4) and the client row offsets live in LDS; per-lane quorum tables
// live in an LDS plane indexed [member][lane] (bank-conflict free).
//
// Reference map:
//   eval_config            Search::compute_stats   fantoch_bote/src/search.rs:262-319
//     Q phase              Bote::quorum_latency    fantoch_bote/src/lib.rs:155-163,169-185
//     leader selection     Bote::best_leader (COV) fantoch_bote/src/lib.rs:99-150
//     client loop          Bote::leaderless        fantoch_bote/src/lib.rs:38-59
//     FPaxos moments       Bote::leader            fantoch_bote/src/lib.rs:67-89
//     score / validity     Search::compute_score   fantoch_bote/src/search.rs:421-472
//   rank enumeration       Search::compute_configs fantoch_bote/src/search.rs:234-260
//                          (permutator combination -> colex ranks)
//   k_single_*             Bote::{leaderless, leader, all_leaders_stats, best_leader}
#include "bote_kernels.hpp"
#include <type_traits>

#include "bote_launch.hpp"
#include "bote_pinned.hpp"

namespace bote {

// ------------------------------------------------------------ LDS carving --
struct Smem {
  uint32_t* mat;     // R*R   latency << 4, row = from
  uint32_t* clioff;  // nc    client row offsets (cli[c] * R)
  uint32_t* srv;     // ns    server region ids
  uint64_t* cs;      // 2*ns  per position: sum_c L[c][srv[p]], sum_c L^2
  uint32_t* cmx;     // ns    per position: max_c L[c][srv[p]] (the MAX keys of FPaxos)
  uint64_t* binom;   // (ns+1)*(N+1)
  uint32_t* qtab;    // N * BD * NLW
  TopkLds tk;        // top MAXOBJ*KP, cand BD, tmp KP, thr MAXOBJ, cnt
};

__host__ __device__ inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// One layout function used by host (sizing) and device (carving).
__host__ __device__ inline size_t smem_layout(const EvalArgs& a, int N, int NLW, uint32_t BD, bool topk,
                                              size_t* off) {
  size_t o = 0;
  off[0] = o; o += (size_t)a.R * a.R * 4;
  off[1] = o; o += (size_t)a.nc * 4;
  off[2] = o; o += (size_t)a.ns * 4;
  o = align_up(o, 16);
  off[3] = o; o += (size_t)a.ns * 16;
  off[4] = o; o += a.cfgs ? 0 : (size_t)(a.ns + 1) * (N + 1) * 8;
  o = align_up(o, 16);
  off[5] = o; o += (size_t)N * BD * NLW * 4;
  o = align_up(o, 16);
  off[6] = o; o += topk ? (size_t)MAXOBJ * KP * 16 : 0;
  off[7] = o; o += topk ? (size_t)BD * 16 : 0;
  off[8] = o; o += topk ? (size_t)KP * 16 : 0;
  off[9] = o; o += topk ? (size_t)MAXOBJ * 16 : 0;
  off[10] = o; o += 48;
  off[11] = o; o += (size_t)a.ns * 4;  // cmx
  return o;
}

template <int N>
__device__ inline Smem carve(const EvalArgs& a, unsigned char* base, int NLW) {
  size_t off[12];
  smem_layout(a, N, NLW, blockDim.x, a.out_top != nullptr, off);
  Smem s;
  s.mat = (uint32_t*)(base + off[0]);
  s.clioff = (uint32_t*)(base + off[1]);
  s.srv = (uint32_t*)(base + off[2]);
  s.cs = (uint64_t*)(base + off[3]);
  s.binom = (uint64_t*)(base + off[4]);
  s.qtab = (uint32_t*)(base + off[5]);
  s.tk.top = (Rec*)(base + off[6]);
  s.tk.cand = (Rec*)(base + off[7]);
  s.tk.tmp = (Rec*)(base + off[8]);
  s.tk.thr = (Rec*)(base + off[9]);
  s.tk.cnt = (int*)(base + off[10]);
  s.cmx = (uint32_t*)(base + off[11]);
  return s;
}

// arr[i] for a lane-varying i without an indexed private array: an OR of
// masked registers (a plain select chain is turned into a scratch lookup).
template <int N>
__device__ __forceinline__ uint32_t sel(const uint32_t (&arr)[N], uint32_t i) {
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) r |= arr[j] & (0u - (uint32_t)(i == (uint32_t)j));
  return r;
}

// --------------------------------------------------------- config result --
// X: the extended key set (slots 10..19 and every leader's FPaxos moments,
// al[f - 1][config-order leader], Input clients); PASSES (EVAL_*): a top-K
// sweep with a percentile objective (EVAL_PCTL) or an MDTM objective
// (EVAL_MDTM, which has the percentile passes too); these have their own
// instantiations: the others keep their code and registers
template <int N, bool X, int PASSES = EVAL_PLAIN>
struct CfgOut {
  static constexpr int NS = X ? NSLOT_X : NSLOT;
  static constexpr bool PCTL = PASSES >= EVAL_PCTL;
  Mom mom[NS];
  uint32_t mx[NS];  // Histogram::max per slot (top-K sweeps only: the MAX keys)
  uint32_t pt[PCTL ? MAXOBJ : 1];  // PCTL: twice Histogram::percentile per percentile objective
  uint64_t mh[PASSES >= EVAL_MDTM ? MAXOBJ : 1];  // EVAL_MDTM: H (mdtm_key) per MDTM objective
  Mom al[X ? 2 : 1][X ? N : 1];
  uint32_t lead_orig;
  double score;
  bool valid;
};

// Slot presence for a config of size N (af2/ff2 need max_f >= 2).
template <int N>
__device__ __forceinline__ bool slot_has(int s) {
  return slot_exists<N>(s);
}

// ------------------------------------------------------------- eval one ---
// Evaluate the configuration whose members are positions p[0..N) of the
// server list (given order = config order).  `oi` is the output row (FULL).
template <int N, bool FULL, bool X, int PASSES = EVAL_PLAIN>
__device__ __forceinline__ void eval_config(const EvalArgs& a, const Smem& s, const uint32_t (&p)[N], bool sorted_in, uint64_t oi,
                            CfgOut<N, X, PASSES>& out) {
  constexpr bool PCTL = PASSES >= EVAL_PCTL;
  using QC = QCfg<N>;
  using QT = QTab<N, X>;
  constexpr int NL = QT::NT;  // leaderless tables: compute_stats' q's, then the extended ones
  constexpr int NLW = (NL + 1) / 2;
  constexpr int P = Pow2<N>::v;
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
  const uint32_t R = a.R, nc = a.nc;

  // --- members, sorted by region id (== name order) for the closest-server
  //     tie-break; `orig` keeps the config order for the leader tie-break.
  uint32_t mk[P];
#pragma unroll
  for (int j = 0; j < N; ++j) mk[j] = (s.srv[p[j]] << 12) | (p[j] << 4) | (uint32_t)j;
#pragma unroll
  for (int j = N; j < P; ++j) mk[j] = 0xFFFFFFFFu;
  if (!sorted_in) sort_network<P>(mk);
  uint32_t mreg[N], mpos[N], morig[N], moff[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    mreg[j] = mk[j] >> 12;
    mpos[j] = (mk[j] >> 4) & 0xFF;
    morig[j] = mk[j] & 15;
    moff[j] = mreg[j] * R;
  }

  // --- Q phase: per member j, the sorted distances to the config (row j of
  //     the config submatrix, self included); colocated closest server.
  uint32_t Qf1[N], Qf2[N], Ql[NL][N], cdk[N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t v[P];
    uint32_t key = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      uint32_t w = s.mat[moff[j] + mreg[k]];
      v[k] = w >> LAT_SHIFT;
      key = min(key, w | (uint32_t)k);
    }
#pragma unroll
    for (int k = N; k < P; ++k) v[k] = 0xFFFFFFFFu;
    sort_network<P>(v);
    Qf1[j] = v[QC::qf1 - 1];
    Qf2[j] = QC::maxf >= 2 ? v[(QC::maxf >= 2 ? QC::qf2 : 1) - 1] : 0;
#pragma unroll
    for (int t = 0; t < NL; ++t) Ql[t][j] = v[QT::q(t) - 1];
    cdk[j] = key;
    // the lane's quorum tables, two u16 per word: word w of member j at
    // qtab[(j * NLW + w) * BD + tid] (bank-conflict free)
#pragma unroll
    for (int w = 0; w < NLW; ++w)
      s.qtab[(j * NLW + w) * BD + tid] = Ql[2 * w][j] | (2 * w + 1 < NL ? (Ql[2 * w + 1 < NL ? 2 * w + 1 : 0][j] << 16) : 0u);
  }

  // --- FPaxos leader: min COV over the Input clients at f = 1 (q = 2),
  //     first in config order on ties.  Exact moments from the per-position
  //     column sums: sum_c (L[c][l] + Q)^k expands in sum_c L and sum_c L^2.
  Mom lm[N];
#pragma unroll
  for (int l = 0; l < N; ++l) {
    uint64_t c1 = s.cs[2 * mpos[l]], c2 = s.cs[2 * mpos[l] + 1], q = Qf1[l];
    lm[l] = leader_mom(c1, c2, nc, q);
  }
  Mom bm = lm[0];
  uint32_t bo = morig[0], bi = 0;
  bool amb = false;
#pragma unroll
  for (int l = 1; l < N; ++l) {
    int c = cov_cmp(lm[l], bm);
    if (c == CMP_AMBIG) {
      amb = true;
    } else if (c == CMP_LT || (c == CMP_EQ && morig[l] < bo)) {
      bm = lm[l];
      bo = morig[l];
      bi = l;
    }
  }
  if (amb) {
    // Near-tie: replay the reference's f64 arithmetic for every leader.
    double cv[N];
#pragma unroll
    for (int l = 0; l < N; ++l) {
      const uint32_t col = mreg[l], q = Qf1[l];
      auto gen = [&](uint32_t c) { return (s.mat[s.clioff[c] + col] >> LAT_SHIFT) + q; };
      cv[l] = ref_cov(gen, nc, lm[l].s1);
    }
    double bc = cv[0];
    bo = morig[0];
    bi = 0;
#pragma unroll
    for (int l = 1; l < N; ++l) {
      int c = f64_cmp(cv[l], bc);
      if (c < 0 || (c == 0 && morig[l] < bo)) {
        bc = cv[l];
        bo = morig[l];
        bi = l;
      }
    }
  }
  const uint32_t lreg = sel(mreg, bi), lpos = sel(mpos, bi);
  const uint32_t lq1 = sel(Qf1, bi), lq2 = sel(Qf2, bi);
  out.lead_orig = bo;

  const uint32_t stride = 5 * nc + 5 * N;
  const bool wv = FULL && a.out_vals != nullptr;  // write per-client values
  uint32_t* ov = wv ? a.out_vals + oi * stride : nullptr;

  // --- Input FPaxos (search.rs:291-302): moments from column sums.
  {
    uint64_t c1 = s.cs[2 * lpos], c2 = s.cs[2 * lpos + 1];
    uint64_t q = lq1;
    out.mom[SLOT_FF1] = leader_mom(c1, c2, nc, q);
    q = lq2;
    out.mom[SLOT_FF2] = leader_mom(c1, c2, nc, q);
    if (!FULL) {  // the worst client of the leader's column, plus the quorum latency
      const uint32_t cm = s.cmx[lpos];
      out.mx[SLOT_FF1] = cm + lq1;
      out.mx[SLOT_FF2] = cm + lq2;
    }
  }

  // --- Colocated keys: clients are the config members (config order).
  {
    uint64_t f1 = 0, f1s = 0, f2 = 0, f2s = 0;
    uint64_t l1[NL], l2[NL];
    uint32_t fm = 0, lm[NL];
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      l1[t] = l2[t] = 0;
      lm[t] = 0;
    }
#pragma unroll
    for (int k = 0; k < N; ++k) {
      uint32_t v = s.mat[moff[k] + lreg] >> LAT_SHIFT;  // ping_latency(client k, leader)
      uint32_t x1 = v + lq1, x2 = v + lq2;
      f1 += x1; f1s += (uint64_t)x1 * x1;
      f2 += x2; f2s += (uint64_t)x2 * x2;
      fm = max(fm, v);
      uint32_t d = cdk[k] >> LAT_SHIFT, js = cdk[k] & 15;
      uint32_t A[NL];
#pragma unroll
      for (int t = 0; t < NL; ++t) {
        A[t] = d + sel(Ql[t], js);
        l1[t] += A[t];
        l2[t] += (uint64_t)A[t] * A[t];
        lm[t] = max(lm[t], A[t]);
      }
      if (wv) {
        uint32_t* oc = ov + 5 * nc;
        uint32_t o = morig[k];
        oc[SLOT_AF1 * N + o] = A[QC::idx_a1];
        oc[SLOT_FF1 * N + o] = x1;
        oc[SLOT_AF2 * N + o] = QC::maxf >= 2 ? A[QC::idx_a2] : 0xFFFFFFFFu;
        oc[SLOT_FF2 * N + o] = QC::maxf >= 2 ? x2 : 0xFFFFFFFFu;
        oc[SLOT_E * N + o] = A[QC::idx_e];
      }
    }
    out.mom[5 + SLOT_FF1] = Mom{f1, f1s, (uint32_t)N};
    out.mom[5 + SLOT_FF2] = Mom{f2, f2s, (uint32_t)N};
    out.mom[5 + SLOT_AF1] = Mom{l1[QC::idx_a1], l2[QC::idx_a1], (uint32_t)N};
    out.mom[5 + SLOT_AF2] = Mom{l1[QC::idx_a2], l2[QC::idx_a2], (uint32_t)N};
    out.mom[5 + SLOT_E] = Mom{l1[QC::idx_e], l2[QC::idx_e], (uint32_t)N};
    if constexpr (X) {
      constexpr int t2 = QT::idx(2), t3 = QT::idx(3) < 0 ? 0 : QT::idx(3), t4 = QT::idx(4) < 0 ? 0 : QT::idx(4);
      out.mom[4 + SLOT_TT1] = Mom{l1[t2], l2[t2], (uint32_t)N};
      out.mom[4 + SLOT_TW1] = Mom{l1[t2], l2[t2], (uint32_t)N};
      out.mom[4 + SLOT_TT2] = Mom{l1[t4], l2[t4], (uint32_t)N};
      out.mom[4 + SLOT_TW2] = Mom{l1[t3], l2[t3], (uint32_t)N};
    }
    if (!FULL) {
      out.mx[5 + SLOT_FF1] = fm + lq1;
      out.mx[5 + SLOT_FF2] = fm + lq2;
      out.mx[5 + SLOT_AF1] = lm[QC::idx_a1];
      out.mx[5 + SLOT_AF2] = lm[QC::idx_a2];
      out.mx[5 + SLOT_E] = lm[QC::idx_e];
      if constexpr (X) {
        constexpr int t2 = QT::idx(2), t3 = QT::idx(3) < 0 ? 0 : QT::idx(3), t4 = QT::idx(4) < 0 ? 0 : QT::idx(4);
        out.mx[4 + SLOT_TT1] = lm[t2];
        out.mx[4 + SLOT_TW1] = lm[t2];
        out.mx[4 + SLOT_TT2] = lm[t4];
        out.mx[4 + SLOT_TW2] = lm[t3];
      }
    }
  }

  // --- Input leaderless: the hot loop.  Per client (wave-uniform): the
  //     nearest member by packed (latency << 4 | member) min, then the
  //     member's quorum latencies from the lane's LDS table.
  {
    uint32_t S1[NL];
    uint64_t S2[NL];
    uint32_t M[NL];
#pragma unroll
    for (int t = 0; t < NL; ++t) { S1[t] = 0; S2[t] = 0; M[t] = 0; }
    for (uint32_t c = 0; c < nc; ++c) {
      const uint32_t off = s.clioff[c];
      uint32_t m = 0xFFFFFFFFu;
#pragma unroll
      for (int k = 0; k < N; ++k) m = min(m, s.mat[off + mreg[k]] | (uint32_t)k);
      const uint32_t js = m & 15, d = m >> LAT_SHIFT;
      uint32_t A[NL];
#pragma unroll
      for (int w = 0; w < NLW; ++w) {
        const uint32_t wd = s.qtab[(js * NLW + w) * BD + tid];
        A[2 * w] = d + (wd & 0xFFFF);
        if (2 * w + 1 < NL) A[2 * w + 1 < NL ? 2 * w + 1 : 0] = d + (wd >> 16);
      }
#pragma unroll
      for (int t = 0; t < NL; ++t) {
        S1[t] += A[t];
        S2[t] += (uint64_t)A[t] * A[t];
        if (!FULL) M[t] = max(M[t], A[t]);
      }
      if (wv) {
        uint32_t v = s.mat[off + lreg] >> LAT_SHIFT;
        ov[SLOT_AF1 * nc + c] = A[QC::idx_a1];
        ov[SLOT_FF1 * nc + c] = v + lq1;
        ov[SLOT_AF2 * nc + c] = QC::maxf >= 2 ? A[QC::idx_a2] : 0xFFFFFFFFu;
        ov[SLOT_FF2 * nc + c] = QC::maxf >= 2 ? v + lq2 : 0xFFFFFFFFu;
        ov[SLOT_E * nc + c] = A[QC::idx_e];
      }
    }
    out.mom[SLOT_AF1] = Mom{S1[QC::idx_a1], S2[QC::idx_a1], nc};
    out.mom[SLOT_AF2] = Mom{S1[QC::idx_a2], S2[QC::idx_a2], nc};
    out.mom[SLOT_E] = Mom{S1[QC::idx_e], S2[QC::idx_e], nc};
    if constexpr (X) {
      // Tempo tiny (2f) and write (f + 1) quorums, Input
      constexpr int t2 = QT::idx(2), t3 = QT::idx(3) < 0 ? 0 : QT::idx(3), t4 = QT::idx(4) < 0 ? 0 : QT::idx(4);
      out.mom[SLOT_TT1] = Mom{S1[t2], S2[t2], nc};
      out.mom[SLOT_TW1] = Mom{S1[t2], S2[t2], nc};
      out.mom[SLOT_TT2] = Mom{S1[t4], S2[t4], nc};
      out.mom[SLOT_TW2] = Mom{S1[t3], S2[t3], nc};
    }
    if (!FULL) {
      out.mx[SLOT_AF1] = M[QC::idx_a1];
      out.mx[SLOT_AF2] = M[QC::idx_a2];
      out.mx[SLOT_E] = M[QC::idx_e];
      if constexpr (X) {
        constexpr int t2 = QT::idx(2), t3 = QT::idx(3) < 0 ? 0 : QT::idx(3), t4 = QT::idx(4) < 0 ? 0 : QT::idx(4);
        out.mx[SLOT_TT1] = M[t2];
        out.mx[SLOT_TW1] = M[t2];
        out.mx[SLOT_TT2] = M[t4];
        out.mx[SLOT_TW2] = M[t3];
      }
    }
  }
  uint32_t flreg[2] = {0, 0}, flq[2] = {0, 0};  // X: the best leaders by mean (region, quorum latency)
  if constexpr (X) {
    // FPaxos all leaders (Bote::all_leaders_stats, lib.rs:129-150), Input
    // clients, q = f + 1, leaders in config order, and the best leader by
    // Stats::Mean (lib.rs:99-121: the first minimum, exact sums)
    uint32_t alm[2][N] = {};  // the leaders' worst clients
    uint32_t alr[N], alq[2][N];  // their regions and quorum latencies
#pragma unroll
    for (int o = 0; o < N; ++o) {
      uint32_t l = 0;
#pragma unroll
      for (int k = 0; k < N; ++k) l = morig[k] == (uint32_t)o ? (uint32_t)k : l;
      const uint32_t pl = sel(mpos, l);
      const uint64_t c1 = s.cs[2 * pl], c2 = s.cs[2 * pl + 1];
      const uint64_t q1 = sel(Qf1, l), q2 = sel(Qf2, l);
      out.al[0][o] = leader_mom(c1, c2, nc, q1);
      out.al[1][o] = leader_mom(c1, c2, nc, q2);
      if constexpr (PCTL) {
        alr[o] = sel(mreg, l);
        alq[0][o] = (uint32_t)q1;
        alq[1][o] = (uint32_t)q2;
      }
      if (!FULL) {
        const uint32_t cm = s.cmx[pl];
        alm[0][o] = cm + (uint32_t)q1;
        alm[1][o] = cm + (uint32_t)q2;
      }
    }
    Mom b1 = out.al[0][0], b2 = out.al[1][0];
    uint32_t m1 = alm[0][0], m2 = alm[1][0];
    if constexpr (PCTL) {
      flreg[0] = flreg[1] = alr[0];
      flq[0] = alq[0][0];
      flq[1] = alq[1][0];
    }
#pragma unroll
    for (int o = 1; o < N; ++o) {
      if (out.al[0][o].s1 < b1.s1) {
        b1 = out.al[0][o];
        m1 = alm[0][o];
        if constexpr (PCTL) {
          flreg[0] = alr[o];
          flq[0] = alq[0][o];
        }
      }
      if (out.al[1][o].s1 < b2.s1) {
        b2 = out.al[1][o];
        m2 = alm[1][o];
        if constexpr (PCTL) {
          flreg[1] = alr[o];
          flq[1] = alq[1][o];
        }
      }
    }
    out.mom[SLOT_FL1] = b1;
    out.mom[SLOT_FL2] = b2;
    if (!FULL) {
      out.mx[SLOT_FL1] = m1;
      out.mx[SLOT_FL2] = m2;
    }
  }

  // --- Percentile objectives (Histogram::percentile, histogram.rs:110-170):
  //     one more pass over the objective's slot (uniform across lanes) per
  //     objective, keeping the slot's PCTL_DEPTH largest values in a sorted
  //     register list that the next objective reuses.  The values are
  //     regenerated as the passes above made them: leaderless from the nearest
  //     member and the lane's quorum table, FPaxos from the leader's column.
  //     MDTM objectives (Histogram::mdtm, histogram.rs:221-235; EVAL_MDTM) take
  //     the same pass with another accumulator: the slot's sum is known by
  //     now, so the values above its mean are summed and counted against the
  //     threshold T = floor(S1 / cnt) (bote_device.hpp mdtm_thr).
  if constexpr (PCTL) {
#pragma unroll 1
    for (int o = 0; o < a.n_obj; ++o) {
      const uint32_t kind = a.obj_kind[o], sl = a.obj_slot[o];
      const bool mdtm = PASSES >= EVAL_MDTM && kind == OBJ_MDTM;
      if (kind < OBJ_PCTL && !mdtm) continue;
      const uint32_t need = kind & PCTL_NEED_MASK;
      uint32_t L[PCTL_DEPTH];  // descending
#pragma unroll
      for (int i = 0; i < PCTL_DEPTH; ++i) L[i] = 0;
      auto put = [&](uint32_t v) {
#pragma unroll
        for (int i = 0; i < PCTL_DEPTH; ++i) {
          const uint32_t hi = max(L[i], v);
          v = min(L[i], v);
          L[i] = hi;
        }
      };
      const bool colocated = (sl >= 5 && sl < 10) || (sl >= 14 && sl < 18);
      // MDTM: A = the sum of max(v - T, 0), B = the number of v > T; both fit
      // 32 bits (v <= 2 * 16383, at most 4096 values)
      MdtmThr mt{0, 0};
      uint32_t mA = 0, mB = 0;
      const uint32_t mcnt = colocated ? (uint32_t)N : nc;
      if constexpr (PASSES >= EVAL_MDTM) {
        if (mdtm) {
          uint32_t s1 = 0;  // (`sl` is uniform: one scalar branch per slot)
#pragma unroll
          for (int q = 0; q < CfgOut<N, X, PASSES>::NS; ++q)
            if ((uint32_t)q == sl) s1 = (uint32_t)out.mom[q].s1;
          mt = mdtm_thr(s1, mcnt);
        }
      }
      auto see = [&](uint32_t v) {
        if constexpr (PASSES >= EVAL_MDTM) {
          if (mdtm) {
            mA += v > mt.T ? v - mt.T : 0u;
            mB += v > mt.T ? 1u : 0u;
            return;
          }
        }
        put(v);
      };
      // the slot's protocol: 0 af1, 1 ff1, 2 af2, 3 ff2, 4 e, then the
      // extended set's 5 tt1, 6 tt2, 7 tw1, 8 tw2, 9 fl1, 10 fl2
      const uint32_t b = sl < 10 ? sl % 5 : sl < 18 ? 5 + (sl - 10) % 4 : 9 + (sl - 18);
      int ti = -1;  // leaderless: the quorum table
      uint32_t lr = lreg, lq = lq1;  // FPaxos: the leader's region and quorum latency
      if (b == 0) ti = QC::idx_a1;
      else if (b == 2) ti = QC::idx_a2;
      else if (b == 4) ti = QC::idx_e;
      else if (b == 3) lq = lq2;
      if constexpr (X) {
        if (b == 5 || b == 7) ti = QT::idx(2);
        else if (b == 6) ti = QT::idx(4) < 0 ? 0 : QT::idx(4);
        else if (b == 8) ti = QT::idx(3) < 0 ? 0 : QT::idx(3);
        else if (b >= 9) {
          lr = b == 9 ? flreg[0] : flreg[1];
          lq = b == 9 ? flq[0] : flq[1];
        }
      }
      if (ti >= 0) {
        const uint32_t w = (uint32_t)ti >> 1, sh = ((uint32_t)ti & 1) * 16;
        auto value = [&](uint32_t m) {  // m: nearest member's (latency << 4 | member)
          return (m >> LAT_SHIFT) + ((s.qtab[((m & 15) * NLW + w) * BD + tid] >> sh) & 0xFFFFu);
        };
        if (colocated) {
#pragma unroll
          for (int k = 0; k < N; ++k) see(value(cdk[k]));
        } else {
          for (uint32_t c = 0; c < nc; ++c) {
            const uint32_t off = s.clioff[c];
            uint32_t m = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < N; ++k) m = min(m, s.mat[off + mreg[k]] | (uint32_t)k);
            see(value(m));
          }
        }
      } else if (colocated) {
#pragma unroll
        for (int k = 0; k < N; ++k) see((s.mat[moff[k] + lr] >> LAT_SHIFT) + lq);
      } else {
        for (uint32_t c = 0; c < nc; ++c) see((s.mat[s.clioff[c] + lr] >> LAT_SHIFT) + lq);
      }
      if constexpr (PASSES >= EVAL_MDTM) {
        if (mdtm) {
          const uint64_t h = mdtm_h(mcnt, mt, mA, mB);
#pragma unroll
          for (int q = 0; q < MAXOBJ; ++q)
            if (q == o) out.mh[q] = h;
          continue;
        }
      }
      // the need-th largest, and the one above it (need <= the slot's count,
      // so neither is a list entry no value reached)
      uint32_t v = 0, up = 0;
#pragma unroll
      for (int i = 0; i < PCTL_DEPTH; ++i) {
        if ((uint32_t)i + 1 == need) v = L[i];
        if ((uint32_t)i + 2 == need) up = L[i];
      }
      const uint32_t twice = (kind & PCTL_WHOLE) ? v + up : 2 * v;
#pragma unroll
      for (int q = 0; q < MAXOBJ; ++q)
        if (q == o) out.pt[q] = twice;
    }
  }

  // --- Search::compute_score (search.rs:421-472), bit-exact.
  out.valid = false;
  out.score = 0.0;
  if (a.want_score) {
    const int fmax = min(N / 2, a.ft_metric);
    bool valid = true;
    double score = 0.0;
#pragma unroll
    for (int f = 1; f <= 2; ++f) {
      if (f > fmax) break;
      const int sa = f == 1 ? SLOT_AF1 : SLOT_AF2, sf = f == 1 ? SLOT_FF1 : SLOT_FF2;
      const Mom& ma = out.mom[sa];
      const Mom& mf = out.mom[sf];
      double fmi = mom_mean(mf) - mom_mean(ma);
      bool fair;
      if (cov_nan(mf) || cov_nan(ma)) {
        fair = false;  // NaN - x >= p is false
      } else {
        int c = CMP_AMBIG;
        if (a.p_fair == 0.0) {
          c = cov_cmp(mf, ma);
          fair = c != CMP_LT;
        } else {
          double d = mom_cov(mf) - mom_cov(ma);
          double tol = 1e-9 * (1.0 + fabs(mom_cov(mf)) + fabs(mom_cov(ma)));
          if (fabs(d - a.p_fair) > tol) c = CMP_EQ;
          fair = d >= a.p_fair;
        }
        if (c == CMP_AMBIG) {
          // replay the reference's f64 covs of ff_f and af_f (Input)
          const uint32_t qfl = f == 1 ? lq1 : lq2;
          auto genf = [&](uint32_t cc) { return (s.mat[s.clioff[cc] + lreg] >> LAT_SHIFT) + qfl; };
          const int ti = f == 1 ? QC::idx_a1 : QC::idx_a2;
          auto gena = [&](uint32_t cc) {
            const uint32_t off = s.clioff[cc];
            uint32_t m = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < N; ++k) m = min(m, s.mat[off + mreg[k]] | (uint32_t)k);
            uint32_t js = m & 15;
            uint32_t q = 0;
#pragma unroll
            for (int t = 0; t < NL; ++t)
              if (t == ti) q = sel(Ql[t], js);
            return (m >> LAT_SHIFT) + q;
          };
          double cf = ref_cov(genf, nc, mf.s1), ca = ref_cov(gena, nc, ma.s1);
          fair = (cf - ca) >= a.p_fair;
        }
      }
      valid = valid && fmi >= a.p_fmean && fair;
      double emi = mom_mean(out.mom[SLOT_E]) - mom_mean(ma);
      if (N == 11 || N == 13) valid = valid && emi >= a.p_emean;
      double t = 30.0 * emi;
      t = fmi + t;
      score = score + t;
    }
    out.valid = valid;
    out.score = score;
  }
}

// ------------------------------------------------------------ the kernel --
// PIN: the pinned variant (bote_pinned.hpp; top-K sweeps of the base key set in
// the rank-range mode).  [rb, re) are pinned ranks: a lane unranks the free
// indices q of its first one, walks `runlen` successors and merges the members
// per step; the digest and the records carry the full colex rank.
template <int N, bool FULL, bool X, int PASSES = EVAL_PLAIN, bool PIN = false>
__global__ void __launch_bounds__(256) eval_kernel(std::conditional_t<PIN, PinEvalArgs, EvalArgs> a) {
  static_assert(!PIN || (!FULL && !X), "the pinned variant is a top-K sweep of the base key set");
  constexpr bool PCTL = PASSES >= EVAL_PCTL;
  static_assert(!(FULL && PCTL), "percentile and MDTM objectives belong to top-K sweeps");
  constexpr int NLW = (QTab<N, X>::NT + 1) / 2;
  constexpr int NS = CfgOut<N, X>::NS;
  extern __shared__ __align__(16) unsigned char smem[];
  if (a.run_if_over && *a.run_if_over <= a.over_cap) return;  // block-uniform, before any barrier
  const Smem s = carve<N>(a, smem, NLW);
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
  const bool topk = !FULL && a.out_top != nullptr;
  if (a.rank_list && *a.rank_count == 0) {
    // the deferred-config fix-up with nothing deferred (the common case):
    // empty lists for the merge, nothing staged (block-uniform)
    if (topk) {
      Rec* dst = a.out_top + (size_t)blockIdx.x * a.n_obj * KP;
      for (uint32_t i = tid; i < (uint32_t)a.n_obj * KP; i += BD) dst[i] = rec_max();
    }
    return;
  }

  // stage the planet, client offsets, server list, column sums, binomials
  for (uint32_t i = tid; i < a.R * a.R; i += BD) s.mat[i] = a.mat[i];
  for (uint32_t i = tid; i < a.nc; i += BD) s.clioff[i] = a.cli[i] * a.R;
  for (uint32_t i = tid; i < a.ns; i += BD) s.srv[i] = a.srv[i];
  if (!a.cfgs)
    for (uint32_t i = tid; i < (a.ns + 1) * (N + 1); i += BD) s.binom[i] = a.binom[i];
  if (topk) topk_init(s.tk, a.n_obj);
  __syncthreads();
  for (uint32_t i = tid; i < a.ns; i += BD) {
    uint64_t c1 = 0, c2 = 0;
    uint32_t cm = 0;
    const uint32_t col = s.srv[i];
    for (uint32_t c = 0; c < a.nc; ++c) {
      uint64_t v = s.mat[s.clioff[c] + col] >> LAT_SHIFT;
      c1 += v;
      c2 += v * v;
      cm = max(cm, (uint32_t)v);
    }
    s.cs[2 * i] = c1;
    s.cs[2 * i + 1] = c2;
    s.cmx[i] = cm;
  }
  __syncthreads();

  uint64_t total = a.re - a.rb;
  if (a.rank_list) {  // deferred configs: the count is known only on the device
    const uint64_t c = *a.rank_count;
    total = c < total ? c : total;
  }
  const uint64_t runlen = a.rank_list ? 1 : a.runlen;
  const uint64_t njobs = (total + runlen - 1) / runlen;
  const uint64_t G = (uint64_t)gridDim.x * BD;
  const uint64_t outer = (njobs + G - 1) / G;
  const bool sorted_in = !a.cfgs && a.srv_sorted;
  uint64_t valid_cnt = 0, digest = 0;

  for (uint64_t it = 0; it < outer; ++it) {
    const uint64_t job = it * G + (uint64_t)blockIdx.x * BD + tid;
    const bool jobok = job < njobs;
    uint64_t rank = a.rb + job * runlen;  // rank or config index
    uint32_t p[N];
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = j;
    uint64_t rend = a.re;
    [[maybe_unused]] uint32_t q[PIN ? N : 1];  // PIN: the free indices
    if constexpr (PIN) {
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = 0;
      if (jobok) pin_unrank<N>(s.binom, a.ns, a.pz, rank, q);
    } else if (jobok) {
      if (a.cfgs) {
#pragma unroll
        for (int j = 0; j < N; ++j) p[j] = a.cfgs[rank * N + j];
      } else {
        if (a.rank_list) {
          rank = a.rank_list[job];
          rend = rank + 1;
        }
        colex_unrank<N>(s.binom, a.ns, rank, p);
      }
    }
    for (uint64_t t = 0; t < runlen; ++t) {
      const bool have = jobok && rank < rend;
      uint64_t frank = rank;  // the config's full colex rank (PIN: `rank` is the pinned rank)
      if constexpr (PIN) {
        if (have) pin_members<N>(s.binom, a.pz, q, p, frank);
      }
      CfgOut<N, X, PASSES> r;
      if (have) {
        eval_config<N, FULL, X, PASSES>(a, s, p, sorted_in, rank - a.rb, r);
        if constexpr (PIN)  // a bounded batch's limits (PinArgs::lim; no bound otherwise)
          r.valid = r.valid && r.mom[SLOT_AF1].s1 < a.pz.lim[0] &&
                    (QCfg<N>::maxf < 2 || r.mom[SLOT_AF2].s1 < a.pz.lim[1]);
        if (r.valid) ++valid_cnt;
        if (a.want_digest) {
          uint32_t h = 0;
#pragma unroll
          for (int sl = 0; sl < NSLOT; ++sl)
            if (slot_has<N>(sl)) h = digest_fold(h, sl, r.mom[sl].s1, r.mom[sl].s2);
          if constexpr (X) {  // the extended key set: every leader, then slots 10..19
#pragma unroll
            for (int f = 0; f < 2; ++f) {
              if (f >= QCfg<N>::maxf) break;
#pragma unroll
              for (int l = 0; l < N; ++l) h = digest_fold_leader(h, f, l, r.al[f][l].s1, r.al[f][l].s2);
            }
#pragma unroll
            for (int sl = 10; sl < 20; ++sl)
              if (slot_has<N>(sl)) h = digest_fold(h, sl, r.mom[sl].s1, r.mom[sl].s2);
          }
          digest += digest_final(frank, r.lead_orig, h);
        }
        if (FULL) {
          const uint64_t oi = rank - a.rb;
          if (a.out_leader) a.out_leader[oi] = r.lead_orig;
#pragma unroll
          for (int sl = 0; sl < NS; ++sl) {
            const bool h = slot_has<N>(sl);
            if (a.out_s1) a.out_s1[oi * NS + sl] = h ? r.mom[sl].s1 : ~0ull;
            if (a.out_s2) a.out_s2[oi * NS + sl] = h ? r.mom[sl].s2 : ~0ull;
            if (a.out_mean) a.out_mean[oi * NS + sl] = h ? mom_mean(r.mom[sl]) : __longlong_as_double(0x7FF8000000000000ll);
            if (a.out_cov) a.out_cov[oi * NS + sl] = h ? mom_cov(r.mom[sl]) : __longlong_as_double(0x7FF8000000000000ll);
          }
          if constexpr (X) {
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
              for (int l = 0; l < N; ++l) {
                const bool h = f < QCfg<N>::maxf;
                if (a.out_al_s1) a.out_al_s1[(oi * 2 + f) * N + l] = h ? r.al[f][l].s1 : ~0ull;
                if (a.out_al_s2) a.out_al_s2[(oi * 2 + f) * N + l] = h ? r.al[f][l].s2 : ~0ull;
              }
          }
          if (a.out_score) a.out_score[oi] = r.score;
          if (a.out_valid) a.out_valid[oi] = r.valid ? 1 : 0;
        }
      }
      if (topk) {
        uint64_t key[MAXOBJ];
        bool ok[MAXOBJ];
#pragma unroll
        for (int o = 0; o < MAXOBJ; ++o) {
          ok[o] = false;
          key[o] = 0;
          if (o < a.n_obj && have) {
            const uint32_t kind = a.obj_kind[o], sl = a.obj_slot[o];
            ok[o] = true;
            if (kind == OBJ_SCORE) {
              ok[o] = r.valid;
              key[o] = ~orderable_f64(r.score);
            } else {
              // `sl` is uniform: one scalar branch per slot keeps r.mom in
              // registers (a select chain here gets turned into scratch).
#pragma unroll
              for (int q = 0; q < NS; ++q)
                if ((uint32_t)q == sl) {
                  if (PCTL && kind >= OBJ_PCTL)
                    key[o] = pctl_key(r.pt[o], r.mom[q].s1);
                  else if (PASSES >= EVAL_MDTM && kind == OBJ_MDTM)
                    key[o] = mdtm_key(r.mh[PASSES >= EVAL_MDTM ? o : 0], r.mom[q].s1);
                  else
                    key[o] = kind == OBJ_MEAN  ? r.mom[q].s1
                             : kind == OBJ_MAX ? max_key(r.mx[q], r.mom[q].s1)
                                               : cov_key(r.mom[q]);
                }
            }
          }
        }
        topk_step(s.tk, a.n_obj, a.K, key, ok, frank);
      }
      if constexpr (PIN) {
        if (have) pin_next<N>(a.ns, a.pz, q);
      } else {
        if (have && !a.cfgs) colex_next<N>(a.ns, p);
      }
      ++rank;
    }
  }

  if (a.out_counters) {
    if (valid_cnt) atomicAdd(&a.out_counters[0], (unsigned long long)valid_cnt);
    if (digest) atomicAdd(&a.out_counters[1], (unsigned long long)digest);
  }
  if (topk) {
    __syncthreads();
    Rec* dst = a.out_top + (size_t)blockIdx.x * a.n_obj * KP;
    for (uint32_t i = tid; i < (uint32_t)a.n_obj * KP; i += BD) dst[i] = s.tk.top[i];
  }
}

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
    NL_CASE(2) NL_CASE(3) NL_CASE(4) NL_CASE(5) NL_CASE(6) NL_CASE(7) NL_CASE(8) NL_CASE(9)
    NL_CASE(10) NL_CASE(11) NL_CASE(12) NL_CASE(13) NL_CASE(14) NL_CASE(15) NL_CASE(16)
#undef NL_CASE
    default: return 0;
  }
  return smem_layout(a, (int)n, (nl + 1) / 2, bd, topk, off);
}

// the kernel for config size n, full outputs or top-K, base or extended keys
// (null: unsupported), for the occupancy query and the launch alike
// `passes` (EVAL_*): the top-K instantiation that also computes percentile
// objectives, or those and MDTM objectives
// `pin`: the pinned variant (bote_pinned.hpp; top-K, base keys): EVAL_PLAIN, or
// EVAL_MDTM for a sweep with a percentile or an MDTM objective (each level has
// the passes of the ones below it)
static const void* eval_fn(uint32_t n, bool full, bool keys, int passes, bool pin) {
  if (pin && (full || keys)) return nullptr;
  switch (n) {
#define FN_CASE(NN)                                                                                             \
  case NN:                                                                                                      \
    if (pin)                                                                                                    \
      return passes != EVAL_PLAIN ? (const void*)eval_kernel<NN, false, false, EVAL_MDTM, true>                 \
                                  : (const void*)eval_kernel<NN, false, false, EVAL_PLAIN, true>;               \
    if (passes >= EVAL_MDTM && !full)                                                                           \
      return keys ? (const void*)eval_kernel<NN, false, true, EVAL_MDTM>                                        \
                  : (const void*)eval_kernel<NN, false, false, EVAL_MDTM>;                                      \
    if (passes == EVAL_PCTL && !full)                                                                           \
      return keys ? (const void*)eval_kernel<NN, false, true, EVAL_PCTL>                                        \
                  : (const void*)eval_kernel<NN, false, false, EVAL_PCTL>;                                      \
    return keys ? (full ? (const void*)eval_kernel<NN, true, true> : (const void*)eval_kernel<NN, false, true>) \
                : (full ? (const void*)eval_kernel<NN, true, false> : (const void*)eval_kernel<NN, false, false>);
    FN_CASE(2) FN_CASE(3) FN_CASE(4) FN_CASE(5) FN_CASE(6) FN_CASE(7) FN_CASE(8) FN_CASE(9)
    FN_CASE(10) FN_CASE(11) FN_CASE(12) FN_CASE(13) FN_CASE(14) FN_CASE(15) FN_CASE(16)
#undef FN_CASE
    default: return nullptr;
  }
}

int eval_occupancy(uint32_t n, bool full, uint32_t bd, size_t shm, bool keys, int passes, bool pin) {
  const void* k = eval_fn(n, full, keys, passes, pin);
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
