// bote_eval.hpp — the generic exact kernel (eval_kernel: any planet, explicit
// configs or colex ranks, full outputs or block top-K lists) as a template.
// Its 150 instantiations are compiled by family in units of their own
// (bote_eval_full.hip, _topk, _pctl, _mdtm, _pinned: N = 2..16 x two variants
// each), so that they build side by side; each unit exports one lookup from
// (n, variant) to its kernels, and eval_fn (bote_kernels.hip) is the only
// place that picks among the lookups.  A kernel's address is taken only in
// the unit that instantiates it.
//
// Work mapping (DESIGN.md "Kernels"): one LANE evaluates one configuration at a
// time; a wavefront holds 64 neighbouring configurations (colex-consecutive
// ranks), so every per-client step is wave-uniform in the client and
// lane-varying only in the config's members.  The R x R latency matrix (stored
// latency << 4) and the client row offsets live in LDS; per-lane quorum tables
// live in an LDS plane indexed [member][lane] (bank-conflict free).
//
// Stage and reference map (eval_config runs the stages in this order):
//   eval_config            Search::compute_stats   fantoch_bote/src/search.rs:262-319
//     sort_members, q_phase  Bote::quorum_latency  fantoch_bote/src/lib.rs:155-163,169-185
//     fpaxos_leader        Bote::best_leader (COV) fantoch_bote/src/lib.rs:99-150
//     input_fpaxos         Bote::leader            fantoch_bote/src/lib.rs:67-89
//     colocated, input_leaderless  Bote::leaderless  fantoch_bote/src/lib.rs:38-59
//     all_leaders (X)      Bote::all_leaders_stats fantoch_bote/src/lib.rs:129-150
//     extra_passes         Histogram::percentile, mdtm  histogram.rs:110-170, 221-235
//     compute_score        Search::compute_score   fantoch_bote/src/search.rs:421-472
//   ConfigCursor           Search::compute_configs fantoch_bote/src/search.rs:234-260
//                          (permutator combination -> colex ranks)
#pragma once
#include "bote_kernels.hpp"
#include <type_traits>

#include "bote_census.hpp"
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

// (TOPK: laid out with the top-K structures whatever a.out_top says: the census variant)
template <int N, bool TOPK = false>
__device__ inline Smem carve(const EvalArgs& a, unsigned char* base, int NLW) {
  size_t off[12];
  smem_layout(a, N, NLW, blockDim.x, TOPK || a.out_top != nullptr, off);
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

// ------------------------------------------------- the stages of a config --
// The config's members sorted by region id (== name order) for the
// closest-server tie-break; `orig` keeps the config order for the leader
// tie-break, `off` is the member's row of the matrix.
template <int N>
struct Members {
  uint32_t reg[N], pos[N], orig[N], off[N];
};

template <int N>
__device__ __forceinline__ void sort_members(const Smem& s, uint32_t R, const uint32_t (&p)[N], bool sorted_in,
                                             Members<N>& m) {
  constexpr int P = Pow2<N>::v;
  uint32_t mk[P];
#pragma unroll
  for (int j = 0; j < N; ++j) mk[j] = (s.srv[p[j]] << 12) | (p[j] << 4) | (uint32_t)j;
#pragma unroll
  for (int j = N; j < P; ++j) mk[j] = 0xFFFFFFFFu;
  if (!sorted_in) sort_network<P>(mk);
#pragma unroll
  for (int j = 0; j < N; ++j) {
    m.reg[j] = mk[j] >> 12;
    m.pos[j] = (mk[j] >> 4) & 0xFF;
    m.orig[j] = mk[j] & 15;
    m.off[j] = m.reg[j] * R;
  }
}

// Q phase: per member j, the sorted distances to the config (row j of the
// config submatrix, self included): the FPaxos quorum latencies f1 / f2, the
// leaderless tables l (compute_stats' q's, then the extended ones) and cdk,
// the colocated closest server as packed (latency << 4 | member).
template <int N, bool X>
struct QPhase {
  static constexpr int NL = QTab<N, X>::NT;
  static constexpr int NLW = (NL + 1) / 2;  // qtab words per member: two u16 tables each
  uint32_t f1[N], f2[N], l[NL][N], cdk[N];
};

template <int N, bool X>
__device__ __forceinline__ void q_phase(const Smem& s, const Members<N>& m, QPhase<N, X>& q) {
  using QC = QCfg<N>;
  using QT = QTab<N, X>;
  constexpr int NL = QPhase<N, X>::NL, NLW = QPhase<N, X>::NLW, P = Pow2<N>::v;
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t v[P];
    uint32_t key = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < N; ++k) {
      uint32_t w = s.mat[m.off[j] + m.reg[k]];
      v[k] = w >> LAT_SHIFT;
      key = min(key, w | (uint32_t)k);
    }
#pragma unroll
    for (int k = N; k < P; ++k) v[k] = 0xFFFFFFFFu;
    sort_network<P>(v);
    q.f1[j] = v[QC::qf1 - 1];
    q.f2[j] = QC::maxf >= 2 ? v[(QC::maxf >= 2 ? QC::qf2 : 1) - 1] : 0;
#pragma unroll
    for (int t = 0; t < NL; ++t) q.l[t][j] = v[QT::q(t) - 1];
    q.cdk[j] = key;
    // the lane's quorum tables, two u16 per word: word w of member j at
    // qtab[(j * NLW + w) * BD + tid] (bank-conflict free)
#pragma unroll
    for (int w = 0; w < NLW; ++w)
      s.qtab[(j * NLW + w) * BD + tid] =
          q.l[2 * w][j] | (2 * w + 1 < NL ? (q.l[2 * w + 1 < NL ? 2 * w + 1 : 0][j] << 16) : 0u);
  }
}

// The nearest member of the client whose matrix row starts at `off`: packed
// (latency << 4 | member) min.
template <int N>
__device__ __forceinline__ uint32_t nearest_member(const Smem& s, const Members<N>& m, uint32_t off) {
  uint32_t k = 0xFFFFFFFFu;
#pragma unroll
  for (int j = 0; j < N; ++j) k = min(k, s.mat[off + m.reg[j]] | (uint32_t)j);
  return k;
}

// FPaxos leader: min COV over the Input clients at f = 1 (q = 2), first in
// config order on ties.  Exact moments from the per-position column sums:
// sum_c (L[c][l] + Q)^k expands in sum_c L and sum_c L^2.
struct Leader {
  uint32_t reg, pos, q1, q2;  // its region, position and quorum latencies (f = 1, 2)
  uint32_t orig;              // its index in config order
};

template <int N, bool X>
__device__ __forceinline__ Leader fpaxos_leader(const Smem& s, uint32_t nc, const Members<N>& m,
                                                const QPhase<N, X>& q) {
  Mom lm[N];
#pragma unroll
  for (int l = 0; l < N; ++l) {
    uint64_t c1 = s.cs[2 * m.pos[l]], c2 = s.cs[2 * m.pos[l] + 1], ql = q.f1[l];
    lm[l] = leader_mom(c1, c2, nc, ql);
  }
  Mom bm = lm[0];
  uint32_t bo = m.orig[0], bi = 0;
  bool amb = false;
#pragma unroll
  for (int l = 1; l < N; ++l) {
    int c = cov_cmp(lm[l], bm);
    if (c == CMP_AMBIG) {
      amb = true;
    } else if (c == CMP_LT || (c == CMP_EQ && m.orig[l] < bo)) {
      bm = lm[l];
      bo = m.orig[l];
      bi = l;
    }
  }
  if (amb) {
    // Near-tie: replay the reference's f64 arithmetic for every leader.
    double cv[N];
#pragma unroll
    for (int l = 0; l < N; ++l) {
      const uint32_t col = m.reg[l], ql = q.f1[l];
      auto gen = [&](uint32_t c) { return (s.mat[s.clioff[c] + col] >> LAT_SHIFT) + ql; };
      cv[l] = ref_cov(gen, nc, lm[l].s1);
    }
    double bc = cv[0];
    bo = m.orig[0];
    bi = 0;
#pragma unroll
    for (int l = 1; l < N; ++l) {
      int c = f64_cmp(cv[l], bc);
      if (c < 0 || (c == 0 && m.orig[l] < bo)) {
        bc = cv[l];
        bo = m.orig[l];
        bi = l;
      }
    }
  }
  return Leader{sel(m.reg, bi), sel(m.pos, bi), sel(q.f1, bi), sel(q.f2, bi), bo};
}

// Input FPaxos (search.rs:291-302): moments from column sums.
template <int N, bool FULL, class Out>
__device__ __forceinline__ void input_fpaxos(const Smem& s, uint32_t nc, const Leader& ld, Out& out) {
  uint64_t c1 = s.cs[2 * ld.pos], c2 = s.cs[2 * ld.pos + 1];
  uint64_t q = ld.q1;
  out.mom[SLOT_FF1] = leader_mom(c1, c2, nc, q);
  q = ld.q2;
  out.mom[SLOT_FF2] = leader_mom(c1, c2, nc, q);
  if (!FULL) {  // the worst client of the leader's column, plus the quorum latency
    const uint32_t cm = s.cmx[ld.pos];
    out.mx[SLOT_FF1] = cm + ld.q1;
    out.mx[SLOT_FF2] = cm + ld.q2;
  }
}

// One placement's leaderless slots (COLO: the Colocated ones) from its
// per-table sums and, for top-K sweeps, maxima over `cnt` clients: af1, af2, e
// and, with X, Tempo's tiny (2f) and write (f + 1) quorums.
template <int N, bool FULL, bool X, bool COLO, class S1, int NL, class Out>
__device__ __forceinline__ void leaderless_slots(const S1 (&s1)[NL], const uint64_t (&s2)[NL],
                                                 const uint32_t (&mx)[NL], uint32_t cnt, Out& out) {
  using QC = QCfg<N>;
  using QT = QTab<N, X>;
  constexpr int B = COLO ? 5 : 0, BX = COLO ? 4 : 0;
  out.mom[B + SLOT_AF1] = Mom{s1[QC::idx_a1], s2[QC::idx_a1], cnt};
  out.mom[B + SLOT_AF2] = Mom{s1[QC::idx_a2], s2[QC::idx_a2], cnt};
  out.mom[B + SLOT_E] = Mom{s1[QC::idx_e], s2[QC::idx_e], cnt};
  if constexpr (X) {
    out.mom[BX + SLOT_TT1] = Mom{s1[QT::tt1], s2[QT::tt1], cnt};
    out.mom[BX + SLOT_TW1] = Mom{s1[QT::tw1], s2[QT::tw1], cnt};
    out.mom[BX + SLOT_TT2] = Mom{s1[QT::tt2], s2[QT::tt2], cnt};
    out.mom[BX + SLOT_TW2] = Mom{s1[QT::tw2], s2[QT::tw2], cnt};
  }
  if (!FULL) {
    out.mx[B + SLOT_AF1] = mx[QC::idx_a1];
    out.mx[B + SLOT_AF2] = mx[QC::idx_a2];
    out.mx[B + SLOT_E] = mx[QC::idx_e];
    if constexpr (X) {
      out.mx[BX + SLOT_TT1] = mx[QT::tt1];
      out.mx[BX + SLOT_TW1] = mx[QT::tw1];
      out.mx[BX + SLOT_TT2] = mx[QT::tt2];
      out.mx[BX + SLOT_TW2] = mx[QT::tw2];
    }
  }
}

// Colocated keys: clients are the config members (config order).  `ov`: the
// config's row of per-client values when `wv` (full outputs with out_vals).
template <int N, bool FULL, bool X, class Out>
__device__ __forceinline__ void colocated(const Smem& s, uint32_t nc, const Members<N>& m, const QPhase<N, X>& q,
                                          const Leader& ld, bool wv, uint32_t* ov, Out& out) {
  using QC = QCfg<N>;
  constexpr int NL = QPhase<N, X>::NL;
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
    uint32_t v = s.mat[m.off[k] + ld.reg] >> LAT_SHIFT;  // ping_latency(client k, leader)
    uint32_t x1 = v + ld.q1, x2 = v + ld.q2;
    f1 += x1; f1s += (uint64_t)x1 * x1;
    f2 += x2; f2s += (uint64_t)x2 * x2;
    fm = max(fm, v);
    uint32_t d = q.cdk[k] >> LAT_SHIFT, js = q.cdk[k] & 15;
    uint32_t A[NL];
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      A[t] = d + sel(q.l[t], js);
      l1[t] += A[t];
      l2[t] += (uint64_t)A[t] * A[t];
      lm[t] = max(lm[t], A[t]);
    }
    if (wv) {
      uint32_t* oc = ov + 5 * nc;
      uint32_t o = m.orig[k];
      oc[SLOT_AF1 * N + o] = A[QC::idx_a1];
      oc[SLOT_FF1 * N + o] = x1;
      oc[SLOT_AF2 * N + o] = QC::maxf >= 2 ? A[QC::idx_a2] : 0xFFFFFFFFu;
      oc[SLOT_FF2 * N + o] = QC::maxf >= 2 ? x2 : 0xFFFFFFFFu;
      oc[SLOT_E * N + o] = A[QC::idx_e];
    }
  }
  out.mom[5 + SLOT_FF1] = Mom{f1, f1s, (uint32_t)N};
  out.mom[5 + SLOT_FF2] = Mom{f2, f2s, (uint32_t)N};
  if (!FULL) {
    out.mx[5 + SLOT_FF1] = fm + ld.q1;
    out.mx[5 + SLOT_FF2] = fm + ld.q2;
  }
  leaderless_slots<N, FULL, X, true>(l1, l2, lm, (uint32_t)N, out);
}

// Input leaderless: the hot loop.  Per client (wave-uniform): the nearest
// member, then the member's quorum latencies from the lane's LDS table.
template <int N, bool FULL, bool X, class Out>
__device__ __forceinline__ void input_leaderless(const Smem& s, uint32_t nc, const Members<N>& m, const Leader& ld,
                                                 bool wv, uint32_t* ov, Out& out) {
  using QC = QCfg<N>;
  constexpr int NL = QPhase<N, X>::NL, NLW = QPhase<N, X>::NLW;
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
  uint32_t S1[NL];
  uint64_t S2[NL];
  uint32_t M[NL];
#pragma unroll
  for (int t = 0; t < NL; ++t) { S1[t] = 0; S2[t] = 0; M[t] = 0; }
  for (uint32_t c = 0; c < nc; ++c) {
    const uint32_t off = s.clioff[c];
    const uint32_t nm = nearest_member<N>(s, m, off);
    const uint32_t js = nm & 15, d = nm >> LAT_SHIFT;
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
      uint32_t v = s.mat[off + ld.reg] >> LAT_SHIFT;
      ov[SLOT_AF1 * nc + c] = A[QC::idx_a1];
      ov[SLOT_FF1 * nc + c] = v + ld.q1;
      ov[SLOT_AF2 * nc + c] = QC::maxf >= 2 ? A[QC::idx_a2] : 0xFFFFFFFFu;
      ov[SLOT_FF2 * nc + c] = QC::maxf >= 2 ? v + ld.q2 : 0xFFFFFFFFu;
      ov[SLOT_E * nc + c] = A[QC::idx_e];
    }
  }
  leaderless_slots<N, FULL, X, false>(S1, S2, M, nc, out);
}

// X: FPaxos all leaders (Bote::all_leaders_stats, lib.rs:129-150), Input
// clients, q = f + 1, leaders in config order, and the best leader by
// Stats::Mean (lib.rs:99-121: the first minimum, exact sums) for f = 1, 2:
// slots fl1 / fl2.  BestLeaders (PCTL only): their regions and quorum latencies.
struct BestLeaders {
  uint32_t reg[2] = {0, 0}, q[2] = {0, 0};
};

template <int N, bool FULL, bool PCTL, class Out>
__device__ __forceinline__ void all_leaders(const Smem& s, uint32_t nc, const Members<N>& m,
                                            const QPhase<N, true>& q, Out& out, BestLeaders& fl) {
  uint32_t alm[2][N] = {};  // the leaders' worst clients
  uint32_t alr[N], alq[2][N];  // their regions and quorum latencies
#pragma unroll
  for (int o = 0; o < N; ++o) {
    uint32_t l = 0;
#pragma unroll
    for (int k = 0; k < N; ++k) l = m.orig[k] == (uint32_t)o ? (uint32_t)k : l;
    const uint32_t pl = sel(m.pos, l);
    const uint64_t c1 = s.cs[2 * pl], c2 = s.cs[2 * pl + 1];
    const uint64_t q1 = sel(q.f1, l), q2 = sel(q.f2, l);
    out.al[0][o] = leader_mom(c1, c2, nc, q1);
    out.al[1][o] = leader_mom(c1, c2, nc, q2);
    if constexpr (PCTL) {
      alr[o] = sel(m.reg, l);
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
    fl.reg[0] = fl.reg[1] = alr[0];
    fl.q[0] = alq[0][0];
    fl.q[1] = alq[1][0];
  }
#pragma unroll
  for (int o = 1; o < N; ++o) {
    if (out.al[0][o].s1 < b1.s1) {
      b1 = out.al[0][o];
      m1 = alm[0][o];
      if constexpr (PCTL) {
        fl.reg[0] = alr[o];
        fl.q[0] = alq[0][o];
      }
    }
    if (out.al[1][o].s1 < b2.s1) {
      b2 = out.al[1][o];
      m2 = alm[1][o];
      if constexpr (PCTL) {
        fl.reg[1] = alr[o];
        fl.q[1] = alq[1][o];
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

// What a slot's values are made of, as the stages above made them: a
// leaderless slot from the nearest member and table `ti` of the lane's quorum
// tables; an FPaxos slot (ti < 0) from the column of leader region `lr` and
// its quorum latency `lq`.  `colocated`: over the members, not the clients.
struct SlotSource {
  int ti;
  uint32_t lr, lq;
  bool colocated;
};

template <int N, bool X>
__device__ __forceinline__ SlotSource slot_source(uint32_t sl, const Leader& ld, const BestLeaders& fl) {
  using QC = QCfg<N>;
  using QT = QTab<N, X>;
  // the slot's protocol: 0 af1, 1 ff1, 2 af2, 3 ff2, 4 e, then the
  // extended set's 5 tt1, 6 tt2, 7 tw1, 8 tw2, 9 fl1, 10 fl2
  const uint32_t b = sl < 10 ? sl % 5 : sl < 18 ? 5 + (sl - 10) % 4 : 9 + (sl - 18);
  SlotSource src{-1, ld.reg, ld.q1, (sl >= 5 && sl < 10) || (sl >= 14 && sl < 18)};
  if (b == 0) src.ti = QC::idx_a1;
  else if (b == 2) src.ti = QC::idx_a2;
  else if (b == 4) src.ti = QC::idx_e;
  else if (b == 3) src.lq = ld.q2;
  if constexpr (X) {
    if (b == 5) src.ti = QT::tt1;
    else if (b == 7) src.ti = QT::tw1;
    else if (b == 6) src.ti = QT::tt2;
    else if (b == 8) src.ti = QT::tw2;
    else if (b >= 9) {
      src.lr = b == 9 ? fl.reg[0] : fl.reg[1];
      src.lq = b == 9 ? fl.q[0] : fl.q[1];
    }
  }
  return src;
}

// Percentile objectives (Histogram::percentile, histogram.rs:110-170): one
// more pass over the objective's slot (uniform across lanes) per objective,
// keeping the slot's PCTL_DEPTH largest values in a sorted register list.  The
// values are regenerated from the slot's source.  MDTM objectives
// (Histogram::mdtm, histogram.rs:221-235; EVAL_MDTM) take the same pass with
// another accumulator: the slot's sum is known by now, so the values above its
// mean are summed and counted against the threshold T = floor(S1 / cnt)
// (bote_device.hpp mdtm_thr).
template <int N, bool X, int PASSES>
__device__ __forceinline__ void extra_passes(const EvalArgs& a, const Smem& s, uint32_t nc, const Members<N>& m,
                                             const QPhase<N, X>& qp, const Leader& ld, const BestLeaders& fl,
                                             CfgOut<N, X, PASSES>& out) {
  constexpr int NLW = QPhase<N, X>::NLW;
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
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
    const SlotSource src = slot_source<N, X>(sl, ld, fl);
    // MDTM: A = the sum of max(v - T, 0), B = the number of v > T; both fit
    // 32 bits (v <= 2 * 16383, at most 4096 values)
    MdtmThr mt{0, 0};
    uint32_t mA = 0, mB = 0;
    const uint32_t mcnt = src.colocated ? (uint32_t)N : nc;
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
    if (src.ti >= 0) {
      const uint32_t w = (uint32_t)src.ti >> 1, sh = ((uint32_t)src.ti & 1) * 16;
      auto value = [&](uint32_t nm) {  // nm: nearest member's (latency << 4 | member)
        return (nm >> LAT_SHIFT) + ((s.qtab[((nm & 15) * NLW + w) * BD + tid] >> sh) & 0xFFFFu);
      };
      if (src.colocated) {
#pragma unroll
        for (int k = 0; k < N; ++k) see(value(qp.cdk[k]));
      } else {
        for (uint32_t c = 0; c < nc; ++c) see(value(nearest_member<N>(s, m, s.clioff[c])));
      }
    } else if (src.colocated) {
#pragma unroll
      for (int k = 0; k < N; ++k) see((s.mat[m.off[k] + src.lr] >> LAT_SHIFT) + src.lq);
    } else {
      for (uint32_t c = 0; c < nc; ++c) see((s.mat[s.clioff[c] + src.lr] >> LAT_SHIFT) + src.lq);
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

// Search::compute_score (search.rs:421-472), bit-exact.
template <int N, bool X, class Out>
__device__ __forceinline__ void compute_score(const EvalArgs& a, const Smem& s, uint32_t nc, const Members<N>& m,
                                              const QPhase<N, X>& qp, const Leader& ld, Out& out) {
  using QC = QCfg<N>;
  constexpr int NL = QPhase<N, X>::NL;
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
          const uint32_t qfl = f == 1 ? ld.q1 : ld.q2;
          auto genf = [&](uint32_t cc) { return (s.mat[s.clioff[cc] + ld.reg] >> LAT_SHIFT) + qfl; };
          const int ti = f == 1 ? QC::idx_a1 : QC::idx_a2;
          auto gena = [&](uint32_t cc) {
            const uint32_t nm = nearest_member<N>(s, m, s.clioff[cc]);
            uint32_t js = nm & 15;
            uint32_t q = 0;
#pragma unroll
            for (int t = 0; t < NL; ++t)
              if (t == ti) q = sel(qp.l[t], js);
            return (nm >> LAT_SHIFT) + q;
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

// ------------------------------------------------------------- eval one ---
// Evaluate the configuration whose members are positions p[0..N) of the
// server list (given order = config order).  `oi` is the output row (FULL).
template <int N, bool FULL, bool X, int PASSES = EVAL_PLAIN>
__device__ __forceinline__ void eval_config(const EvalArgs& a, const Smem& s, const uint32_t (&p)[N], bool sorted_in,
                                            uint64_t oi, CfgOut<N, X, PASSES>& out) {
  const uint32_t nc = a.nc;
  Members<N> m;
  sort_members<N>(s, a.R, p, sorted_in, m);
  QPhase<N, X> q;
  q_phase<N, X>(s, m, q);
  const Leader ld = fpaxos_leader<N, X>(s, nc, m, q);
  out.lead_orig = ld.orig;

  const uint32_t stride = 5 * nc + 5 * N;
  const bool wv = FULL && a.out_vals != nullptr;  // write per-client values
  uint32_t* ov = wv ? a.out_vals + oi * stride : nullptr;

  input_fpaxos<N, FULL>(s, nc, ld, out);
  colocated<N, FULL, X>(s, nc, m, q, ld, wv, ov, out);
  input_leaderless<N, FULL, X>(s, nc, m, ld, wv, ov, out);
  BestLeaders fl;
  if constexpr (X) all_leaders<N, FULL, (PASSES >= EVAL_PCTL)>(s, nc, m, q, out, fl);
  if constexpr (PASSES >= EVAL_PCTL) extra_passes<N, X, PASSES>(a, s, nc, m, q, ld, fl, out);
  compute_score<N, X>(a, s, nc, m, q, ld, out);
}

// ---------------------------------------------------- the kernel's stages --
// Stage the planet, client offsets, server list and (rank modes) binomials,
// then the per-position column sums and maxima over the clients.
template <int N>
__device__ __forceinline__ void stage_planet(const EvalArgs& a, const Smem& s, bool ranks, bool topk) {
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
  for (uint32_t i = tid; i < a.R * a.R; i += BD) s.mat[i] = a.mat[i];
  for (uint32_t i = tid; i < a.nc; i += BD) s.clioff[i] = a.cli[i] * a.R;
  for (uint32_t i = tid; i < a.ns; i += BD) s.srv[i] = a.srv[i];
  if (ranks)
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
}

// A lane's walk over its configs: the one place that knows the four ways of
// enumerating them.  Explicit lists (a.cfgs: [rb, re) are config indices),
// rank ranges (`runlen` consecutive colex ranks per lane job), the deferred
// rank list (a.rank_list, its length read on the device: one rank per job) and
// pinned ranks (PIN, bote_pinned.hpp: [rb, re) are pinned ranks; a lane
// unranks the free indices q of its first one, walks `runlen` successors and
// merges the members per step).
// The walk's state stays in the kernel's own variables, which the functions
// take by reference: p (the config's members, positions), q (PIN: the free
// indices), rank (rank, pinned rank or config index) and rend (the end of the
// lane's run).  As members of the cursor the same code costs the kernels 6 to
// 8 VGPRs (N = 8: 248 -> 254, and the percentile kernel's 256 -> 261 a wave).
template <int N, bool PIN>
struct ConfigCursor {
  using Args = std::conditional_t<PIN, PinEvalArgs, EvalArgs>;
  static constexpr int NQ = PIN ? N : 1;

  __device__ __forceinline__ static bool unranks(const Args& a) { return !a.cfgs; }  // (needs the binomials)
  __device__ __forceinline__ static bool sorted_in(const Args& a) { return !a.cfgs && a.srv_sorted; }
  __device__ __forceinline__ static uint64_t runlen(const Args& a) { return a.rank_list ? 1 : a.runlen; }
  __device__ __forceinline__ static uint64_t total(const Args& a) {
    uint64_t total = a.re - a.rb;
    if (a.rank_list) {  // deferred configs: the count is known only on the device
      const uint64_t c = *a.rank_count;
      total = c < total ? c : total;
    }
    return total;
  }

  __device__ __forceinline__ static void first(const Args& a, const Smem& s, uint64_t job, bool jobok,
                                               uint32_t (&p)[N], uint32_t (&q)[NQ], uint64_t& rank, uint64_t& rend) {
    rank = a.rb + job * runlen(a);
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = j;
    rend = a.re;
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
  }
  // the step's config: `frank` comes in as `rank` and leaves as the config's
  // full colex rank (PIN: `rank` is the pinned rank, and the members are merged here)
  __device__ __forceinline__ static void members(const Args& a, const Smem& s, bool have, const uint32_t (&q)[NQ],
                                                 uint32_t (&p)[N], uint64_t& frank) {
    if constexpr (PIN) {
      if (have) pin_members<N>(s.binom, a.pz, q, p, frank);
    }
  }
  __device__ __forceinline__ static void next(const Args& a, bool have, uint32_t (&p)[N], uint32_t (&q)[NQ],
                                              uint64_t& rank) {
    if constexpr (PIN) {
      if (have) pin_next<N>(a.ns, a.pz, q);
    } else {
      if (have && !a.cfgs) colex_next<N>(a.ns, p);
    }
    ++rank;
  }
};

// the config's term of the digest: every slot's moments and its leader
template <int N, bool X, class Out>
__device__ __forceinline__ uint64_t config_digest(const Out& r, uint64_t frank) {
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
  return digest_final(frank, r.lead_orig, h);
}

// FULL: row `oi` of every output the caller asked for
template <int N, bool X, class Out>
__device__ __forceinline__ void write_full(const EvalArgs& a, uint64_t oi, const Out& r) {
  constexpr int NS = Out::NS;
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

// the census variant's sink in the top-K regions it takes (eval_kernel below)
__device__ __forceinline__ CensusLds census_lds(const Smem& s) {
  return CensusLds{s.tk.top, (unsigned long long*)s.tk.cand};
}

// ------------------------------------------------------------ the kernel --
// PIN: the pinned variant (bote_pinned.hpp; top-K sweeps of the base key set in
// the rank-range mode); the digest and the records carry the full colex rank.
// CENSUS: the census variant (bote_census.hpp; base key set, ranks or the
// deferred rank list): the objectives' keys as a top-K sweep builds them, and
// census_step in place of topk_step.  It is laid out as a top-K sweep (the
// launcher sizes it so): the thresholds take the lists' region (tk.top, at
// least n_obj x KP records), the bins the candidate buffer's (tk.cand, 16 B per
// thread of the block).
// CON: the constrained variant (ConArgs, bote_kernels.hpp; base key set, ranks
// or the deferred rank list, unpinned): a.n_obj key entries, the objectives and
// then the constraints, built alike; a config whose trailing keys are not all
// within their bounds offers nothing, the others are counted (con_admit).  The
// lists are the first n_lists entries'.  The valid count and the digest are the
// unconstrained sweep's.
template <int N, bool FULL, bool X, int PASSES = EVAL_PLAIN, bool PIN = false, bool CENSUS = false, bool CON = false>
__global__ void __launch_bounds__(256)
    eval_kernel(std::conditional_t<CON, ConEvalArgs,
                                   std::conditional_t<CENSUS, CensusEvalArgs, std::conditional_t<PIN, PinEvalArgs, EvalArgs>>> a) {
  static_assert(!CON || (!FULL && !X && !PIN && !CENSUS), "the constrained variant is an unpinned top-K sweep of the base key set");
  static_assert(!PIN || (!FULL && !X), "the pinned variant is a top-K sweep of the base key set");
  static_assert(!CENSUS || (!FULL && !X && !PIN), "the census variant sweeps ranks of the base key set");
  static_assert(CENSUS_T <= KP && CENSUS_T * 8 * MAXOBJ <= 256 * 16, "the census sink fits the top-K regions it takes");
  constexpr bool PCTL = PASSES >= EVAL_PCTL;
  static_assert(!(FULL && PCTL), "percentile and MDTM objectives belong to top-K sweeps");
  constexpr int NS = CfgOut<N, X>::NS;
  using Cursor = ConfigCursor<N, PIN>;
  extern __shared__ __align__(16) unsigned char smem[];
  if (a.run_if_over && *a.run_if_over <= a.over_cap) return;  // block-uniform, before any barrier
  const Smem s = carve<N, CENSUS>(a, smem, QPhase<N, X>::NLW);
  const uint32_t BD = blockDim.x, tid = threadIdx.x;
  const bool topk = CENSUS || (!FULL && a.out_top != nullptr);
  if constexpr (CENSUS) {
    // a fix-up over a queue that overflowed: the fallback counts the whole range (block-uniform)
    if (a.rank_list && *a.rank_count > a.re - a.rb) return;
  }
  if (a.rank_list && *a.rank_count == 0) {
    // the deferred-config fix-up with nothing deferred (the common case):
    // empty lists for the merge, nothing staged (block-uniform)
    if (topk && !CENSUS) {
      Rec* dst = a.out_top + (size_t)blockIdx.x * list_count<CON>(a) * KP;
      for (uint32_t i = tid; i < (uint32_t)list_count<CON>(a) * KP; i += BD) dst[i] = rec_max();
    }
    return;
  }
  if constexpr (CENSUS) census_init(census_lds(s), nullptr, a.cz, a.n_obj, a.obj_kind);  // (published by the stage's barriers)
  stage_planet<N>(a, s, Cursor::unranks(a), topk && !CENSUS);
  if constexpr (CON) {
    if (topk) con_init(s.tk, a.cz);
    __syncthreads();
  }

  const uint64_t total = Cursor::total(a), runlen = Cursor::runlen(a);
  const uint64_t njobs = (total + runlen - 1) / runlen;
  const uint64_t G = (uint64_t)gridDim.x * BD;
  const uint64_t outer = (njobs + G - 1) / G;
  const bool sorted_in = Cursor::sorted_in(a);
  uint64_t valid_cnt = 0, digest = 0;
  [[maybe_unused]] std::conditional_t<CON, uint64_t, char> adm_cnt{};  // CON: the lane's admitted configs

  for (uint64_t it = 0; it < outer; ++it) {
    const uint64_t job = it * G + (uint64_t)blockIdx.x * BD + tid;
    const bool jobok = job < njobs;
    uint32_t p[N];
    [[maybe_unused]] uint32_t q[Cursor::NQ];
    uint64_t rank, rend;
    Cursor::first(a, s, job, jobok, p, q, rank, rend);
    for (uint64_t t = 0; t < runlen; ++t) {
      const bool have = jobok && rank < rend;
      uint64_t frank = rank;
      Cursor::members(a, s, have, q, p, frank);
      CfgOut<N, X, PASSES> r;
      if (have) {
        eval_config<N, FULL, X, PASSES>(a, s, p, sorted_in, rank - a.rb, r);
        if constexpr (PIN)  // a bounded batch's limits (PinArgs::lim; no bound otherwise)
          r.valid = r.valid && r.mom[SLOT_AF1].s1 < a.pz.lim[0] &&
                    (QCfg<N>::maxf < 2 || r.mom[SLOT_AF2].s1 < a.pz.lim[1]);
        if (r.valid) ++valid_cnt;
        if (a.want_digest) digest += config_digest<N, X>(r, frank);
        if (FULL) write_full<N, X>(a, rank - a.rb, r);
      }
      if (topk) {
        uint64_t key[MAXOBJ];
        bool ok[MAXOBJ];
        // The objectives' keys stay in the kernel body: as a stage function
        // over (r, key, ok) the slot branches below compile differently (the
        // N = 2 and 3 kernels take 129 and 131 VGPRs, not 114 and 118, and
        // lose a wave per SIMD; DESIGN.md §4 "The generic kernel").
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
        if constexpr (CON) {
          if (have && con_admit(s.tk, list_count<CON>(a), a.n_obj, key, ok)) ++adm_cnt;
        }
        if constexpr (CENSUS) census_step(census_lds(s), a.n_obj, a.cz.T, key, ok, frank);
        else topk_step(s.tk, list_count<CON>(a), a.K, key, ok, frank);
      }
      Cursor::next(a, have, p, q, rank);
    }
  }

  if (a.out_counters) {
    if (valid_cnt) atomicAdd(&a.out_counters[0], (unsigned long long)valid_cnt);
    if (digest) atomicAdd(&a.out_counters[1], (unsigned long long)digest);
  }
  if constexpr (CON) {
    if (adm_cnt) atomicAdd(a.cz.admitted, (unsigned long long)adm_cnt);
  }
  if constexpr (CENSUS) {
    __syncthreads();
    census_flush(census_lds(s), a.cz, a.n_obj);
  } else if (topk) {
    __syncthreads();
    Rec* dst = a.out_top + (size_t)blockIdx.x * list_count<CON>(a) * KP;
    for (uint32_t i = tid; i < (uint32_t)list_count<CON>(a) * KP; i += BD) dst[i] = s.tk.top[i];
  }
}

// ------------------------------------------------- the families' lookups --
// The config sizes every family is instantiated for (BOTE_MAX_N = 16).
#define BOTE_EVAL_SIZES(M) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15) M(16)

// One per unit, hidden: the unit's kernel for config size n (30 each: every
// size x base / extended keys, or for the pinned ones x EVAL_PLAIN /
// EVAL_MDTM), or null.  The units instantiate their kernels explicitly.
#define BOTE_HIDDEN __attribute__((visibility("hidden")))
BOTE_HIDDEN const void* eval_fn_full(uint32_t n, bool keys);    // bote_eval_full.hip: full outputs
BOTE_HIDDEN const void* eval_fn_topk(uint32_t n, bool keys);    // bote_eval_topk.hip: top-K, EVAL_PLAIN
BOTE_HIDDEN const void* eval_fn_pctl(uint32_t n, bool keys);    // bote_eval_pctl.hip: top-K, EVAL_PCTL
BOTE_HIDDEN const void* eval_fn_mdtm(uint32_t n, bool keys);    // bote_eval_mdtm.hip: top-K, EVAL_MDTM
BOTE_HIDDEN const void* eval_fn_pinned(uint32_t n, bool passes);  // bote_eval_pinned.hip: EVAL_MDTM (passes) or EVAL_PLAIN
BOTE_HIDDEN const void* eval_fn_census(uint32_t n, bool passes);  // bote_eval_census.hip: the same two, census sink
BOTE_HIDDEN const void* eval_fn_con(uint32_t n, bool passes);     // bote_eval_con.hip: the same two, constrained

}  // namespace bote
