// bote_sweep.hip — the fast-path sweep kernel (gfx950): exhaustive search over
// colex ranks with a block top-K, for planets that meet the fast-path
// preconditions checked on the host (bote_capi_sweep.hip, fast_eligible):
//   * every latency <= 4095 (packed u16 keys: latency << 4 | member)
//   * the server set is "simple": self latency 0, latency between two servers
//     > 0 (a colocated client's nearest server is itself)
//   * servers in name order, >= 2 clients, min_fairness_fpaxos_improv == 0
// Anything else runs the generic kernel (bote_eval.hpp), which is also the
// exact path for the rare configs this kernel defers (COV near-ties).
//
// Data layout in LDS (DESIGN.md "Data layout"):
//   CQT[t][g]  uint2 = 4 x u16 (latency << 4) from clients 4g..4g+3 to region
//              t; column stride (nq + 1) * 8 bytes, an odd number of 8-byte
//              slots, so distinct columns spread over the ds_read_b64 banks.
//   RQT        the same layout with ALL regions as the rows (== CQT when the
//              client list is 0..R-1): L[a][b] = RQT[b][a >> 2].u16[a & 3].
//   qtab       per lane and member: packed leaderless quorum latencies,
//              plane-major [member][lane] (conflict-free).
//
// Per config (one lane; reference functions in bote_eval.hpp's header):
// quorum latencies by sorting each member's off-diagonal distances; FPaxos
// leader by exact-COV comparison (variance is shift invariant, so leader l's
// V = nc*sum(L^2) - (sum L)^2 of its column, precomputed per position); the
// Input leaderless keys by the packed client-quad loop; compute_score validity
// by integer / f64-margin decisions; digest; block top-K.
//
// The file in order: LDS regions; the client loop; the stages; the kernel,
// which is the sequence of the stages; the launcher.  What a variant FAST_*
// adds to a config is in its tail carrier (bote_fast_tail.hpp), which has one
// hook per stage.
//
// The constrained variant's instantiations are a unit of their own
// (bote_sweep_con.hip, which defines BOTE_FAST_CON_UNIT and includes this
// file): it compiles beside this one and leaves out what is not a template.
#include "bote_census.hpp"
#include "bote_fast_tail.hpp"
#include "bote_launch.hpp"
#include "bote_pinned.hpp"


namespace bote {


// The workgroup's LDS regions (byte offsets, in this order), fast_layout
struct FastLds {
  size_t qtab;      // first: offsets stay small
  size_t cqt, rqt;  // rqt == cqt unless the launch has a matrix of its own for it
  size_t srv, cs1, cs2, vcol, binom;
  size_t top, cand, tmp, thr, cnt;  // TopkLds (cnt: 1 + MAXOBJ counters)
  size_t cmax, c4, ch;              // the tail variants' columns (TailCols)
  size_t cthr, cbin;                // the census variant's thresholds and bins (CensusLds), in place of top, cand and tmp
  size_t total;
};

__host__ __device__ inline FastLds fast_layout(const FastArgs& a, int N, int NLW, int tail, bool census = false) {
  const auto a16 = [](size_t o) { return (o + 15) & ~(size_t)15; };
  FastLds l;
  size_t o = 0;
  l.qtab = o; o += (size_t)N * FAST_BD * NLW * 4;
  l.cqt = o; o += (size_t)a.R * a.cq_stride * 8;
  l.rqt = a.rq_separate ? o : l.cqt; o += a.rq_separate ? (size_t)a.R * a.rq_stride * 8 : 0;
  l.srv = o; o += (size_t)a.ns * 4;
  l.cs1 = o; o += (size_t)a.ns * 4;
  o = a16(o);
  l.cs2 = o; o += (size_t)a.ns * 8;
  l.vcol = o; o += (size_t)a.ns * 8;
  l.binom = o; o += (size_t)(a.ns + 1) * (N + 1) * 8;
  o = a16(o);
  l.top = o; o += census ? 0 : (size_t)a.n_obj * KP * 16;
  l.cand = o; o += census ? 0 : (size_t)FAST_BD * 16;
  l.tmp = o; o += census ? 0 : (size_t)KP * 16;
  l.thr = o; o += (size_t)MAXOBJ * 16;
  l.cnt = o; o += 48;
  l.cmax = o; o += tail == FAST_MAX ? (size_t)a.ns * 4 : 0;
  l.c4 = o; o += tail == FAST_LIST ? (size_t)a.ns * 8 : 0;  // (8-byte aligned: every region above is)
  l.ch = o; o += tail == FAST_MDTM ? (size_t)a.ns * 8 : 0;  // (the same)
  if (census) o = a16(o);
  l.cthr = o; o += census ? (size_t)a.n_obj * CENSUS_T * 16 : 0;
  l.cbin = o; o += census ? (size_t)a.n_obj * CENSUS_T * 8 : 0;
  l.total = o;
  return l;
}

// The batch variant keeps the unit's two limits (PinArgs::lim) in the last two
// of the 12 words reserved at `cnt` (16-byte aligned; the top-K uses 1 + MAXOBJ):
// no variant's layout changes.
constexpr int BATCH_LIM_WORD = 10;
static_assert(1 + MAXOBJ <= BATCH_LIM_WORD && (BATCH_LIM_WORD + 2) * 4 <= 48 && BATCH_LIM_WORD % 2 == 0,
              "the limits follow the top-K counters inside the reserved 48 bytes, 8-byte aligned");

#ifndef BOTE_FAST_CON_UNIT
size_t fast_smem_bytes(const FastArgs& a, uint32_t n, int tail, bool census) {
  int nl = 0;
  switch (n) {
#define NL_CASE(NN) case NN: nl = QCfg<NN>::NL; break;
    NL_CASE(2) NL_CASE(3) NL_CASE(4) NL_CASE(5) NL_CASE(6) NL_CASE(7) NL_CASE(8) NL_CASE(9)
    NL_CASE(10) NL_CASE(11) NL_CASE(12) NL_CASE(13) NL_CASE(14) NL_CASE(15) NL_CASE(16)
#undef NL_CASE
    default: return 0;
  }
  return fast_layout(a, (int)n, nl <= 2 ? 1 : 2, tail, census).total;
}
#endif

struct FastSmem {
  unsigned char* base;  // dynamic LDS base; byte offsets below are relative to it
  uint32_t cqt, rqt, qtab;
  uint32_t* srv;
  uint32_t* cs1;
  uint64_t* cs2;
  double* vcol;
  uint64_t* binom;
  TailCols tc;  // the tail variants' columns
  TopkLds tk;
  CensusLds cl;  // the census variant's sink (tk.top, tk.cand and tmp are empty then; tk.thr holds the screen's keys)
};

__device__ __forceinline__ FastSmem fast_smem(const FastLds& l, unsigned char* smem) {
  FastSmem s;
  s.base = smem;
  s.qtab = (uint32_t)l.qtab;
  s.cqt = (uint32_t)l.cqt;
  s.rqt = (uint32_t)l.rqt;
  s.srv = (uint32_t*)(smem + l.srv);
  s.cs1 = (uint32_t*)(smem + l.cs1);
  s.cs2 = (uint64_t*)(smem + l.cs2);
  s.vcol = (double*)(smem + l.vcol);
  s.binom = (uint64_t*)(smem + l.binom);
  s.tc.cmax = (uint32_t*)(smem + l.cmax);
  s.tc.c4 = (uint2*)(smem + l.c4);
  s.tc.ch = (uint64_t*)(smem + l.ch);
  s.tk.top = (Rec*)(smem + l.top);
  s.tk.cand = (Rec*)(smem + l.cand);
  s.tk.tmp = (Rec*)(smem + l.tmp);
  s.tk.thr = (Rec*)(smem + l.thr);
  s.tk.cnt = (int*)(smem + l.cnt);
  s.cl.thr = (Rec*)(smem + l.cthr);
  s.cl.bin = (unsigned long long*)(smem + l.cbin);
  return s;
}

// ------------------------------------------------------------ hot loop ----
// one call of f per leaderless table t with the quad's quorum latencies of it,
// clients 0, 1 in ql01 and 2, 3 in ql23 (v_perm out of the qtab words)
template <int NL, int NQ, class F>
__device__ __forceinline__ void each_table(const uint32_t (&q)[NQ], F&& f) {
  f(0, __builtin_amdgcn_perm(q[1], q[0], 0x05040100u), __builtin_amdgcn_perm(q[3], q[2], 0x05040100u));
  if (NL >= 2)
    f(NL >= 2 ? 1 : 0, __builtin_amdgcn_perm(q[1], q[0], 0x07060302u), __builtin_amdgcn_perm(q[3], q[2], 0x07060302u));
  if (NL == 3)
    f(NL - 1, __builtin_amdgcn_perm(q[NQ - 3], q[NQ - 4], 0x05040100u),
      __builtin_amdgcn_perm(q[NQ - 1], q[NQ - 2], 0x05040100u));
}
// the remainder quad's masks: `rem` = 1..3 live clients
__device__ __forceinline__ uint32_t rem_lo(uint32_t rem) { return rem >= 2 ? ~0u : 0x0000FFFFu; }
__device__ __forceinline__ uint32_t rem_hi(uint32_t rem) { return rem == 3 ? 0x0000FFFFu : 0u; }

// Input leaderless keys over client quads.  Per quad and member: one
// ds_read_b64 (4 clients), a packed OR of the member index and a packed min
// (v_pk_min_u16: ties go to the lower member = the lower name); per client:
// one qtab read for the nearest member's quorum latencies; packed adds and
// v_dot2_u32_u16 accumulate the sum and the sum of squares.  Squares are
// accumulated in 32 bits and flushed to 64 bits every `flushQ` quads.  `lp` is
// the tail carrier's loop part (TailLoop): it sees every masked half quad, and
// one with a second pass sees them again after the sums are known.
template <int N, int NL, class LP>
__device__ __forceinline__ void client_quads(const unsigned char* B, uint32_t cqt, uint32_t nq, uint32_t rem,
                                             uint32_t flushQ, const uint32_t (&colT)[N], uint32_t qlane,
                                             uint32_t (&S1)[NL], uint64_t (&S2)[NL], LP& lp) {
  const us2 ones = {1, 1};
  constexpr int NQ = NL == 3 ? 8 : 4;  // qtab words per quad
  uint32_t s2[NL];
#pragma unroll
  for (int t = 0; t < NL; ++t) {
    S1[t] = 0;
    S2[t] = 0;
    s2[t] = 0;
  }
  lp.init();
  uint32_t col[N];
#pragma unroll
  for (int j = 0; j < N; ++j) col[j] = cqt + colT[j];

  // stage 1: the quad's N member columns
  auto load = [&](uint32_t g8, uint2 (&w)[N]) {
#pragma unroll
    for (int j = 0; j < N; ++j) w[j] = ld64(B, col[j] + g8);
  };
  // stage 2: nearest member per client (packed min of latency<<4 | member)
  auto nearest = [&](const uint2 (&w)[N], us2& lo, us2& hi) {
    lo = as_us2(w[0].x);
    hi = as_us2(w[0].y);
#pragma unroll
    for (int j = 1; j < N; ++j) {
      const us2 J = {(unsigned short)j, (unsigned short)j};
      lo = __builtin_elementwise_min(lo, as_us2(w[j].x) | J);
      hi = __builtin_elementwise_min(hi, as_us2(w[j].y) | J);
    }
  };
  // stage 3a: the nearest members' quorum latencies (qtab sits at LDS offset
  // 0, so qlane < 2^QSH and the member plane offset can be OR-ed in);
  // `plane2`: the third table's plane too (a second pass skips it when that
  // table does not need one)
  auto qread = [&](us2 lo, us2 hi, uint32_t (&q)[NQ], bool plane2 = true) {
    constexpr uint32_t QM = 15u << QSH;
    const uint32_t L = as_u32(lo), H = as_u32(hi);
    q[0] = ld32(B, ((L << QSH) & QM) | qlane);
    q[1] = ld32(B, ((L >> (16 - QSH)) & QM) | qlane);
    q[2] = ld32(B, ((H << QSH) & QM) | qlane);
    q[3] = ld32(B, ((H >> (16 - QSH)) & QM) | qlane);
    if (NL == 3 && plane2) {
      const uint32_t P2 = (uint32_t)N << QSH;  // second plane follows the first
      q[NQ - 4] = ld32(B, qlane + P2 + ((L & 15u) << QSH));
      q[NQ - 3] = ld32(B, qlane + P2 + (((L >> 16) & 15u) << QSH));
      q[NQ - 2] = ld32(B, qlane + P2 + ((H & 15u) << QSH));
      q[NQ - 1] = ld32(B, qlane + P2 + (((H >> 16) & 15u) << QSH));
    }
  };
  // stage 3b: client latency = distance + quorum latency; S1 and S2 by dot2
  auto accum = [&](us2 lo, us2 hi, const uint32_t (&q)[NQ], uint32_t mlo, uint32_t mhi) {
    const us2 dlo = lo >> (us2)4, dhi = hi >> (us2)4;
    each_table<NL>(q, [&](int t, uint32_t ql01, uint32_t ql23) {
      const us2 a01 = lat2(dlo, ql01, mlo), a23 = lat2(dhi, ql23, mhi);
      S1[t] = __builtin_amdgcn_udot2(a01, ones, S1[t], false);
      S1[t] = __builtin_amdgcn_udot2(a23, ones, S1[t], false);
      s2[t] = __builtin_amdgcn_udot2(a01, a01, s2[t], false);
      s2[t] = __builtin_amdgcn_udot2(a23, a23, s2[t], false);
      lp.acc(t, a01, a23);
    });
  };
  auto quad = [&](uint32_t g8, uint32_t mlo, uint32_t mhi) {
    uint2 w[N];
    uint32_t q[NQ];
    us2 lo, hi;
    load(g8, w);
    nearest(w, lo, hi);
    qread(lo, hi, q);
    accum(lo, hi, q, mlo, mhi);
  };
  auto flush = [&]() {
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      S2[t] += s2[t];
      s2[t] = 0;
    }
  };

  uint32_t g = 0;
  if (N <= 8 && flushQ >= 2) {
    // Software-pipelined pairs: the next pair's 2N column reads (merged
    // into ds_read2_b64) are in flight while this pair's qtab reads and
    // sums run; the scheduling barriers keep the compiler from serialising
    // the reads behind their first use, which it otherwise does to save
    // registers under the 128-VGPR cap.
    const uint32_t np = nq >> 1;
    const uint32_t fp = flushQ >> 1;
    if (np) {
      uint2 wa[N], wb[N];
      load(0, wa);
      load(8, wb);
      uint32_t k = 0;
      for (uint32_t p = 0; p < np; ++p) {
        us2 loA, hiA, loB, hiB;
        nearest(wa, loA, hiA);
        nearest(wb, loB, hiB);
        uint32_t qA[NQ], qB[NQ];
        qread(loA, hiA, qA);
        qread(loB, hiB, qB);
        const uint32_t gn = min(p + 1, np - 1) * 16;
        load(gn, wa);
        load(gn + 8, wb);
        __builtin_amdgcn_sched_barrier(0);
        accum(loA, hiA, qA, ~0u, ~0u);
        accum(loB, hiB, qB, ~0u, ~0u);
        if (++k == fp) {
          flush();
          k = 0;
        }
      }
      flush();
      g = np << 1;
    }
  }
  for (uint32_t g0 = g; g0 < nq; g0 += flushQ) {
    const uint32_t ge = min(nq, g0 + flushQ);
    for (g = g0; g < ge; ++g) quad(g * 8, ~0u, ~0u);
    flush();
  }
  if (rem) {
    quad(nq * 8, rem_lo(rem), rem_hi(rem));
    flush();
  }
  lp.finish();
  if constexpr (LP::two_pass) {
    if (lp.begin2(S1)) {
      auto quad2 = [&](uint32_t g8, uint32_t mlo, uint32_t mhi) {
        uint2 w[N];
        uint32_t q[NQ] = {};
        us2 lo, hi;
        load(g8, w);
        nearest(w, lo, hi);
        qread(lo, hi, q, lp.third_plane());
        const us2 dlo = lo >> (us2)4, dhi = hi >> (us2)4;
        each_table<NL>(q, [&](int t, uint32_t ql01, uint32_t ql23) { lp.above(t, dlo, dhi, ql01, ql23, mlo, mhi); });
      };
      for (uint32_t g2 = 0; g2 < nq; ++g2) quad2(g2 * 8, ~0u, ~0u);
      if (rem) quad2(nq * 8, rem_lo(rem), rem_hi(rem));
      lp.end2();
    }
  }
}

// ------------------------------------------------------------ the stages --
// quad matrices, server list, binomials into LDS, and the empty block top-K
// (CENSUS: no lists; the kernel fills the census sink itself)
template <int N, bool CENSUS = false>
__device__ __forceinline__ void stage_lds(const FastArgs& a, const FastSmem& s, uint32_t tid) {
  const uint32_t cw = a.R * a.cq_stride * 2;  // 32-bit words
  const uint32_t* src = (const uint32_t*)a.cqt;
  uint32_t* dst = (uint32_t*)(s.base + s.cqt);
  for (uint32_t i = tid; i < cw; i += FAST_BD) dst[i] = src[i];
  if (a.rq_separate) {
    const uint32_t rw = a.R * a.rq_stride * 2;
    const uint32_t* rs = (const uint32_t*)a.rqt;
    uint32_t* rd = (uint32_t*)(s.base + s.rqt);
    for (uint32_t i = tid; i < rw; i += FAST_BD) rd[i] = rs[i];
  }
  for (uint32_t i = tid; i < a.ns; i += FAST_BD) s.srv[i] = a.srv[i];
  for (uint32_t i = tid; i < (a.ns + 1) * (N + 1); i += FAST_BD) s.binom[i] = a.binom[i];
  if constexpr (!CENSUS) topk_init(s.tk, a.n_obj);
  __syncthreads();
}

// per position: its client column's sum, sum of squares and V, and the tail variant's column
template <class TL>
__device__ __forceinline__ void position_sums(const FastArgs& a, const FastSmem& s, uint32_t tid) {
  for (uint32_t i = tid; i < a.ns; i += FAST_BD) {
    const uint32_t col = s.cqt + s.srv[i] * a.cq_stride * 8;
    uint64_t c1 = 0, c2 = 0;
    for (uint32_t c = 0; c < a.nc; ++c) {
      const uint64_t v = client_lat(s.base, col, c);
      c1 += v;
      c2 += v * v;
    }
    TL::column(s.tc, s.base, col, a.nc, (uint32_t)c1, i);  // (a pass of its own: once per block)
    s.cs1[i] = (uint32_t)c1;
    s.cs2[i] = c2;
    s.vcol[i] = (double)((uint64_t)a.nc * c2 - c1 * c1);  // exact: < 2^53
  }
  __syncthreads();
}

// The member stage: a lane's walk over `runlen` consecutive ranks.  Unpinned,
// the members p[] are the colex config of the rank.  PIN: the pinned variant
// (bote_pinned.hpp; FAST_PLAIN only).  [rb, re) are pinned ranks; a lane walks
// them over the free indices q and re-merges the members per step.  The full
// colex rank is computed with the members, always: the digest, a record
// offered to the top-K and a deferred config's queue entry carry it, and
// everything after p[N] is the code of the unpinned kernel.  PIN is a mode
// (PIN_*, bote_kernels.hpp): PIN_ONE takes the pinned set `z` from the kernarg,
// PIN_BATCH the set of the unit at hand, loaded from the batch's device table
// (the kernel below); both walk it the same way.
template <int N, int PIN>
struct Members {
  using Args = std::conditional_t<PIN == PIN_BATCH, BatchFastArgs, std::conditional_t<PIN == PIN_ONE, PinFastArgs, FastArgs>>;
  uint32_t p[N];
  [[maybe_unused]] uint32_t q[PIN ? N : 1];  // PIN: the free indices (one unused word otherwise)

  __device__ __forceinline__ void start(const uint64_t* binom, uint32_t ns, const PinArgs& z, bool jobok,
                                        uint64_t rank) {
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = j;
    if constexpr (PIN != PIN_NONE) {
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = 0;
      if (jobok) pin_unrank<N>(binom, ns, z, rank, q);
    } else {
      if (jobok) colex_unrank<N>(binom, ns, rank, p);
    }
  }
  // the members of the config at hand; `frank` comes in as the rank and leaves as the full colex rank
  __device__ __forceinline__ void config(const uint64_t* binom, const PinArgs& z, bool have, uint64_t& frank) {
    if constexpr (PIN != PIN_NONE) {
      if (have) pin_members<N>(binom, z, q, p, frank);
    }
  }
  __device__ __forceinline__ void next(uint32_t ns, const PinArgs& z, bool live) {
    if constexpr (PIN != PIN_NONE) {
      if (live) pin_next<N>(ns, z, q);
    } else {
      if (live) colex_next<N>(ns, p);
    }
  }
};

// Q phase: sorted off-diagonal distances of each member's row -> the members'
// FPaxos quorum latencies Q2, Q3, their leaderless ones into the lane's qtab
// planes, and the colocated leaderless sums cS1, cS2
template <int N, class TL>
__device__ __forceinline__ void q_phase(const FastArgs& a, unsigned char* smem, const uint32_t (&colR)[N],
                                        const uint32_t (&rowq)[N], uint32_t qlane, uint32_t (&Q2)[N],
                                        uint32_t (&Q3)[N], uint32_t (&cS1)[TL::NL], uint32_t (&cS2)[TL::NL], TL& tl) {
  using QC = QCfg<N>;
  constexpr int NL = QC::NL;
  constexpr int P = Pow2<N - 1>::v;  // off-diagonal row values, padded
  const unsigned char* B = smem;
#pragma unroll
  for (int t = 0; t < NL; ++t) cS1[t] = cS2[t] = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t v[P];
    int t = 0;
    if (ABLATE(a, 2)) {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (k != j) v[t++] = colR[k] + rowq[j] + k;
    } else {
#pragma unroll
      for (int k = 0; k < N; ++k)
        if (k != j) v[t++] = ld16(B, colR[k] + rowq[j]) >> LAT_SHIFT;
    }
#pragma unroll
    for (int k = N - 1; k < P; ++k) v[k] = 0xFFFFFFFFu;
    sort_network<P>(v);
    // the row's q-th smallest (self = 0 first) is the (q-1)-th off-diagonal
    Q2[j] = v[0];
    Q3[j] = QC::maxf >= 2 ? v[QC::maxf >= 2 ? 1 : 0] : 0u;
    uint32_t ql[NL];
#pragma unroll
    for (int t2 = 0; t2 < NL; ++t2) {
      ql[t2] = v[QC::lq(t2) - 2];
      cS1[t2] += ql[t2];
      cS2[t2] += ql[t2] * ql[t2];
      tl.q_value(t2, ql[t2]);
    }
    *(uint32_t*)(smem + qlane + ((uint32_t)j << QSH)) = ql[0] | (NL >= 2 ? ql[NL >= 2 ? 1 : 0] << 16 : 0u);
    if (NL == 3) *(uint32_t*)(smem + qlane + ((uint32_t)(N + j) << QSH)) = ql[NL - 1];
    // one member row at a time: keeps the row's reads and sort network
    // from being interleaved with the next rows (register pressure)
    __builtin_amdgcn_sched_barrier(0);
  }
}

// the FPaxos leader: its member index, position, quorum latencies and RQT column, carried along
struct Leader {
  uint32_t bi, lp, lq2, lq3, lcol;
};
// FPaxos leader (f = 1, q = 2, min COV, first in config order).  False when a
// comparison is within the ambiguity band: the caller defers the config.
template <int N>
__device__ __forceinline__ bool fpaxos_leader(const FastSmem& s, const uint32_t (&p)[N], uint32_t nc,
                                              const uint32_t (&Q2)[N], const uint32_t (&Q3)[N],
                                              const uint32_t (&colR)[N], Leader& ld) {
  bool amb = false;
  ld = Leader{0, p[0], Q2[0], Q3[0], colR[0]};
  uint32_t c1 = s.cs1[p[0]];
  double bS = (double)(c1 + nc * Q2[0]);
  bS = bS * bS;
  double bV = s.vcol[p[0]];
#pragma unroll
  for (int l = 1; l < N; ++l) {
    const double V = s.vcol[p[l]];
    double S = (double)(s.cs1[p[l]] + nc * Q2[l]);
    S = S * S;
    const double x = V * bS, y = bV * S;  // cov_l^2 < cov_best^2  <=>  x < y
    const bool zero = (V == 0.0) && (bV == 0.0);
    const double d = x - y, tol = 0x1p-32 * fmax(x, y);
    if (!zero && fabs(d) <= tol) amb = true;
    if (!zero && d < -tol) {
      bS = S;
      bV = V;
      ld = Leader{(uint32_t)l, p[l], Q2[l], Q3[l], colR[l]};
    }
  }
  return !amb;
}

// Input leaderless: the hot loop (first, so little is live across it)
template <int N, class TL>
__device__ __forceinline__ void input_leaderless(const unsigned char* B, uint32_t cqt, uint32_t nc,
                                                 const uint32_t (&colT)[N], uint32_t qlane, Mom (&mom)[NSLOT], TL& tl,
                                                 const FastArgs& a, uint64_t (&key)[MAXOBJ], bool (&ok)[MAXOBJ]) {
  using QC = QCfg<N>;
  constexpr int NL = QC::NL;
  uint32_t S1[NL];
  uint64_t S2[NL];
  typename TL::Loop L = tl.loop(nc);
  client_quads<N, NL>(B, cqt, ABLATE(a, 1) ? 0u : nc >> 2, ABLATE(a, 1) ? 0u : nc & 3, a.s2_flush, colT, qlane, S1, S2,
                      L);
  if (ABLATE(a, 1)) {  // timing only: non-degenerate dummy sums (nothing defers)
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      S1[t] = 1000u + colT[0] + t;
      S2[t] = (uint64_t)S1[t] * S1[t] + 12345u;
    }
  }
  mom[SLOT_AF1] = Mom{S1[QC::idx_a1], S2[QC::idx_a1], nc};
  mom[SLOT_AF2] = Mom{S1[QC::idx_a2], S2[QC::idx_a2], nc};
  mom[SLOT_E] = Mom{S1[QC::idx_e], S2[QC::idx_e], nc};
  tl.leaderless(L, TailKeys{a, mom, key, ok});
}

// Input FPaxos: moments from the leader column's sums
template <class TL>
__device__ __forceinline__ void input_fpaxos(const FastSmem& s, const Leader& ld, uint32_t nc, Mom (&mom)[NSLOT],
                                             TL& tl, const FastArgs& a, uint64_t (&key)[MAXOBJ], bool (&ok)[MAXOBJ]) {
  mom[SLOT_FF1] = leader_mom(s.cs1[ld.lp], s.cs2[ld.lp], nc, ld.lq2);
  mom[SLOT_FF2] = leader_mom(s.cs1[ld.lp], s.cs2[ld.lp], nc, ld.lq3);
  tl.fpaxos(s.tc, ld.lp, ld.lq2, ld.lq3, TailKeys{a, mom, key, ok});
}

// Colocated: leaderless values are the members' own quorum latencies;
// FPaxos reads the leader's column of the config submatrix.
template <int N, class TL>
__device__ __forceinline__ void colocated(const unsigned char* B, const Leader& ld, const uint32_t (&rowq)[N],
                                          uint32_t qlane, const uint32_t (&cS1)[TL::NL], const uint32_t (&cS2)[TL::NL],
                                          Mom (&mom)[NSLOT], TL& tl, const FastArgs& a, uint64_t (&key)[MAXOBJ],
                                          bool (&ok)[MAXOBJ]) {
  using QC = QCfg<N>;
  uint32_t f1 = 0, f1s = 0, f2 = 0, f2s = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const uint32_t v = ld16(B, ld.lcol + rowq[k]) >> LAT_SHIFT;
    const uint32_t x1 = v + ld.lq2, x2 = v + ld.lq3;
    f1 += x1;
    f1s += x1 * x1;
    f2 += x2;
    f2s += x2 * x2;
  }
  mom[5 + SLOT_FF1] = Mom{f1, f1s, (uint32_t)N};
  mom[5 + SLOT_FF2] = Mom{f2, f2s, (uint32_t)N};
  mom[5 + SLOT_AF1] = Mom{cS1[QC::idx_a1], cS2[QC::idx_a1], (uint32_t)N};
  mom[5 + SLOT_AF2] = Mom{cS1[QC::idx_a2], cS2[QC::idx_a2], (uint32_t)N};
  mom[5 + SLOT_E] = Mom{cS1[QC::idx_e], cS2[QC::idx_e], (uint32_t)N};
  tl.colocated_fpaxos(B, ld.lcol, rowq, f1, ld.lq2, ld.lq3, TailKeys{a, mom, key, ok});
  tl.colocated_leaderless(B, qlane, cS1, TailKeys{a, mom, key, ok});
}

// ---------------------------------------------------------- the kernel ----
// The stages above in order; what a variant adds is in its carrier (Tail) and
// in the member stage (Members).  PIN_BATCH (FAST_PLAIN): the workgroup stages
// the planet once, then walks the batch's units blockIdx.x, += gridDim.x
// (BatchArgs): per unit its own rank range and pinned set, a fresh block top-K
// and fresh valid and digest sums, the unit's list slot and the set's counters.
// CENSUS (FAST_PLAIN, unpinned; bote_census.hpp): the stages are the same up to
// and including finish_config, which screens SCORE and COV keys with the
// launch's largest thresholds; the sink is census_step in place of topk_step
// and a flush of counts in place of the list dump.  A deferred config offers
// no key (ok[] stays false), so it is counted for no objective here and for
// every one by the generic kernel's census variant over the queue.
// CON (unpinned; ConArgs, bote_kernels.hpp): the constrained variant.  The
// launch's key entries are its objectives, then its constraints; the stages
// build every entry's key alike.  After finish_config the trailing keys are
// compared with their bounds (con_admit): a rejected config withdraws its
// offers, an admitted one is counted.  A deferred config is neither: the
// generic kernel's constrained variant decides it over the queue.  The block
// top-K, the list dump and the merges see the first n_lists entries only.
template <int N, int TAIL, int PIN = PIN_NONE, bool CENSUS = false, bool CON = false>
__global__ void __launch_bounds__(FAST_BD, 4)
    sweep_fast_kernel(std::conditional_t<CON, ConFastArgs,
                                         std::conditional_t<CENSUS, CensusFastArgs, typename Members<N, PIN>::Args>> a) {
  using TL = Tail<N, TAIL>;
  static_assert(!CON || (PIN == PIN_NONE && !CENSUS), "the constrained variant is an unpinned top-K sweep");
  static_assert(PIN == PIN_NONE || TL::plain, "the pinned variants compute SCORE, MEAN and COV objectives");
  static_assert(!CENSUS || (PIN == PIN_NONE && TL::plain), "the census variant is unpinned and computes SCORE, MEAN and COV objectives");
  constexpr bool BATCH = PIN == PIN_BATCH;
  constexpr int NL = TL::NL;
  extern __shared__ __align__(16) unsigned char smem[];
  const FastSmem s = fast_smem(fast_layout(a, N, NL <= 2 ? 1 : 2, TAIL, CENSUS), smem);
  const uint32_t tid = threadIdx.x;
  const unsigned char* B = smem;

  stage_lds<N, CENSUS>(a, s, tid);
  if constexpr (CENSUS) census_init(s.cl, s.tk.thr, a.cz, a.n_obj, a.obj_kind);  // (published by the next stage's barrier)
  if constexpr (CON) con_init(s.tk, a.cz);  // (after stage_lds' barrier; published by the next stage's)
  position_sums<TL>(a, s, tid);

  const uint32_t cstride = a.cq_stride * 8;  // bytes per CQT column
  const uint32_t rstride = a.rq_stride * 8;
  const uint32_t nc = a.nc;
  const uint32_t qlane = s.qtab + tid * 4;
  const double pnc1 = a.p_fmean * (double)nc, pnc2 = a.p_emean * (double)nc;
  const uint32_t tail_slots = TL::slots(a);
  // the rank range at hand and the lane jobs' spacing: the launch's, or the unit's
  uint64_t rb = a.rb, re = a.re, runlen = a.runlen;
  uint64_t G = (uint64_t)gridDim.x * FAST_BD, first = (uint64_t)blockIdx.x * FAST_BD + tid;
  [[maybe_unused]] uint32_t unit = blockIdx.x, set = 0;  // (block-uniform)
  [[maybe_unused]] PinArgs zb{};                         // BATCH: the unit's pinned set
  const PinArgs& pz = [&]() -> const PinArgs& {
    if constexpr (PIN == PIN_ONE) return a.pz;
    else return zb;
  }();
  Rec* dst = a.out_top + (size_t)blockIdx.x * list_count<CON>(a) * KP;
  unsigned long long* counters = a.out_counters;
  if constexpr (BATCH) {
    if (unit >= a.bz.n_sets * a.bz.slices) return;  // (the launcher's grid is at most the units)
    G = FAST_BD;
    first = tid;
    runlen = a.bz.runlen;
  }
  bool more = false;  // BATCH: another unit for this workgroup
  do {
    if constexpr (BATCH) {
      set = unit / a.bz.slices;
      const uint32_t sl = unit - set * a.bz.slices;
      rb = min((uint64_t)sl * a.bz.slice_len, a.bz.ptotal);
      re = min(rb + a.bz.slice_len, a.bz.ptotal);
      zb = a.bz.sets[set];  // (uniform loads)
      dst = a.out_top + ((size_t)set * BATCH_SET_LISTS + sl) * a.n_obj * KP;
      counters = a.out_counters + 2 * (size_t)set;
      // the unit's limits (PinArgs::lim), written once per unit into the two
      // spare words of the top-K counters' region and read back per config:
      // no scalar stays live over the unit for them.  (The last unit's configs
      // are done: every wave has passed the barrier before its list dump.)
      if (tid == 0) *(uint2*)(s.tk.cnt + BATCH_LIM_WORD) = make_uint2(zb.lim[0], zb.lim[1]);
      if (unit != blockIdx.x) {  // the last unit's list is out: a fresh top-K
        __syncthreads();
        topk_init(s.tk, a.n_obj);
      }
      __syncthreads();
    }
    const uint64_t total = re - rb;
    const uint64_t njobs = (total + runlen - 1) / runlen;
    const uint64_t outer = (njobs + G - 1) / G;
    uint64_t valid_cnt = 0, digest = 0;
    [[maybe_unused]] Only<CON, uint64_t> adm_cnt{};  // CON: the lane's admitted configs

    for (uint64_t it = 0; it < outer; ++it) {
      const uint64_t job = it * G + first;
      const bool jobok = job < njobs;
      uint64_t rank = rb + job * runlen;
      Members<N, PIN> mb;
      mb.start(s.binom, a.ns, pz, jobok, rank);
      for (uint64_t tt = 0; tt < runlen; ++tt) {
        bool have = jobok && rank < re;
        uint64_t frank = rank;  // the config's full colex rank
        mb.config(s.binom, pz, have, frank);
        uint64_t key[MAXOBJ];
        bool ok[MAXOBJ];
#pragma unroll
        for (int o = 0; o < MAXOBJ; ++o) {
          key[o] = 0;
          ok[o] = false;
        }
        // a deferred config goes to the exact generic kernel (bote_sweep_launch; BATCH: the
        // count alone matters, a batch that deferred any config is recomputed on that kernel)
        auto defer = [&]() { defer_rank(a, frank); };
        if (have) {
          // ---- members (positions ascending == names ascending)
          uint32_t colT[N], colR[N], rowq[N];
#pragma unroll
          for (int j = 0; j < N; ++j) {
            const uint32_t r = a.srv_identity ? mb.p[j] : s.srv[mb.p[j]];
            colT[j] = r * cstride;
            colR[j] = s.rqt + r * rstride;
            rowq[j] = (r >> 2) * 8 + (r & 3) * 2;
          }
          TL tl(tail_slots);
          uint32_t Q2[N], Q3[N], cS1[NL], cS2[NL];
          q_phase<N>(a, smem, colR, rowq, qlane, Q2, Q3, cS1, cS2, tl);
          Leader ld;
          if (!fpaxos_leader<N>(s, mb.p, nc, Q2, Q3, colR, ld)) {
            defer();
            have = false;
          }
          if (have) {
            Mom mom[NSLOT];
            input_leaderless<N>(B, s.cqt, nc, colT, qlane, mom, tl, a, key, ok);
            input_fpaxos(s, ld, nc, mom, tl, a, key, ok);
            colocated<N>(B, ld, rowq, qlane, cS1, cS2, mom, tl, a, key, ok);
            tl.build_keys(ld.lq2, ld.lq3, TailKeys{a, mom, key, ok});
            bool pre_valid = true;  // BATCH: the set's limits on the Atlas sums
            if constexpr (BATCH) {
              const uint2 lim = *(const uint2*)(s.tk.cnt + BATCH_LIM_WORD);
              pre_valid = (uint32_t)mom[SLOT_AF1].s1 < lim.x && (QCfg<N>::maxf < 2 || (uint32_t)mom[SLOT_AF2].s1 < lim.y);
            }
            if (!finish_config<N, TAIL>(a, mom, s.vcol[ld.lp], ld.bi, frank, s.tk.thr, pnc1, pnc2, valid_cnt, digest,
                                        key, ok, pre_valid)) {
              defer();
              have = false;
              TL::withdraw(ok);
            }
            if constexpr (CON) {
              if (have && con_admit(s.tk, list_count<CON>(a), a.n_obj, key, ok)) ++adm_cnt;
            }
          }
        }
        if constexpr (CENSUS) census_step(s.cl, a.n_obj, a.cz.T, key, ok, frank);
        else if (!ABLATE(a, 4)) topk_step(s.tk, list_count<CON>(a), a.K, key, ok, frank);
        mb.next(a.ns, pz, jobok && rank < re);
        ++rank;
      }
    }
    if constexpr (BATCH) {  // one add per wave: the sets' counters take a unit's adds at once
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        valid_cnt += (uint64_t)__shfl_xor((long long)valid_cnt, d);
        digest += (uint64_t)__shfl_xor((long long)digest, d);
      }
      if (tid & 63) valid_cnt = digest = 0;
    }
    if (valid_cnt) atomicAdd(&counters[0], (unsigned long long)valid_cnt);
    if (digest) atomicAdd(&counters[1], (unsigned long long)digest);
    if constexpr (CON) {
      if (adm_cnt) atomicAdd(a.cz.admitted, (unsigned long long)adm_cnt);
    }
    __syncthreads();
    if constexpr (CENSUS) census_flush(s.cl, a.cz, a.n_obj);
    else
      for (uint32_t i = tid; i < (uint32_t)list_count<CON>(a) * KP; i += FAST_BD) dst[i] = s.tk.top[i];
    if constexpr (BATCH) more = (unit += gridDim.x) < a.bz.n_sets * a.bz.slices;
  } while (more);
}

// ------------------------------------------------------------- launcher ---
// the constrained variant for config size n (null: not built for `tail`), defined by its own unit
__attribute__((visibility("hidden"))) const void* fast_fn_con(uint32_t n, int tail);
#ifdef BOTE_FAST_CON_UNIT
const void* fast_fn_con(uint32_t n, int tail) {
  switch (n) {
#define FN_CASE(NN)                                                                                      \
  case NN:                                                                                               \
    return tail == FAST_MDTM   ? (const void*)sweep_fast_kernel<NN, FAST_MDTM, PIN_NONE, false, true>    \
           : tail == FAST_LIST ? (const void*)sweep_fast_kernel<NN, FAST_LIST, PIN_NONE, false, true>    \
           : tail == FAST_MAX  ? (const void*)sweep_fast_kernel<NN, FAST_MAX, PIN_NONE, false, true>     \
                               : (const void*)sweep_fast_kernel<NN, FAST_PLAIN, PIN_NONE, false, true>;
    FN_CASE(2) FN_CASE(3) FN_CASE(4) FN_CASE(5) FN_CASE(6) FN_CASE(7) FN_CASE(8) FN_CASE(9)
    FN_CASE(10) FN_CASE(11) FN_CASE(12) FN_CASE(13) FN_CASE(14) FN_CASE(15) FN_CASE(16)
#undef FN_CASE
    default: return nullptr;
  }
}
#else
// the kernel for config size n (null: unsupported; the pinned and the batch
// variant, pin = PIN_*, are FAST_PLAIN only), for the occupancy query and the
// launch alike
static const void* fast_fn(uint32_t n, int tail, int pin, bool census = false) {
  switch (n) {
#define FN_CASE(NN)                                                                  \
  case NN:                                                                           \
    if (census)                                                                      \
      return tail == FAST_PLAIN && pin == PIN_NONE                                   \
                 ? (const void*)sweep_fast_kernel<NN, FAST_PLAIN, PIN_NONE, true>    \
                 : nullptr;                                                          \
    if (pin == PIN_BATCH) return tail == FAST_PLAIN ? (const void*)sweep_fast_kernel<NN, FAST_PLAIN, PIN_BATCH> : nullptr; \
    if (pin == PIN_ONE) return tail == FAST_PLAIN ? (const void*)sweep_fast_kernel<NN, FAST_PLAIN, PIN_ONE> : nullptr; \
    return tail == FAST_MDTM   ? (const void*)sweep_fast_kernel<NN, FAST_MDTM>       \
           : tail == FAST_LIST ? (const void*)sweep_fast_kernel<NN, FAST_LIST>       \
           : tail == FAST_MAX  ? (const void*)sweep_fast_kernel<NN, FAST_MAX>        \
                              : (const void*)sweep_fast_kernel<NN, FAST_PLAIN>;
    FN_CASE(2) FN_CASE(3) FN_CASE(4) FN_CASE(5) FN_CASE(6) FN_CASE(7) FN_CASE(8) FN_CASE(9)
    FN_CASE(10) FN_CASE(11) FN_CASE(12) FN_CASE(13) FN_CASE(14) FN_CASE(15) FN_CASE(16)
#undef FN_CASE
    default: return nullptr;
  }
}

int fast_occupancy(uint32_t n, int tail, int pin, size_t shm, bool census, bool con) {
  const void* k = con ? (pin == PIN_NONE && !census ? fast_fn_con(n, tail) : nullptr) : fast_fn(n, tail, pin, census);
  return k ? kernel_occupancy(k, FAST_BD, shm, 1) : 0;
}

bool fast_has_constrained(uint32_t n, int tail) { return fast_fn_con(n, tail) != nullptr; }

hipError_t launch_fast(const FastArgs& a, uint32_t n, int tail, const PinArgs* pin, uint32_t grid, size_t shm,
                       hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn(n, tail, pin ? PIN_ONE : PIN_NONE);
  if (!k) return hipErrorInvalidValue;
  if (!pin) return launch_kernel(k, a, grid, FAST_BD, shm, st, e0, e1);
  PinFastArgs pa{};
  static_cast<FastArgs&>(pa) = a;
  pa.pz = *pin;
  return launch_kernel(k, pa, grid, FAST_BD, shm, st, e0, e1);
}

hipError_t launch_fast_con(const FastArgs& a, uint32_t n, int tail, const ConArgs& z, uint32_t grid, size_t shm,
                           hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn_con(n, tail);
  if (!k || !z.admitted || a.n_obj > MAXOBJ || z.n_lists > (uint32_t)a.n_obj) return hipErrorInvalidValue;
  ConFastArgs ca{};
  static_cast<FastArgs&>(ca) = a;
  ca.cz = z;
  return launch_kernel(k, ca, grid, FAST_BD, shm, st, e0, e1);
}

hipError_t launch_fast_census(const FastArgs& a, uint32_t n, const CensusArgs& z, uint32_t grid, size_t shm,
                              hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn(n, FAST_PLAIN, PIN_NONE, true);
  if (!k || !z.thr || !z.below || z.T == 0 || z.T > (uint32_t)CENSUS_T) return hipErrorInvalidValue;
  CensusFastArgs ca{};
  static_cast<FastArgs&>(ca) = a;
  ca.cz = z;
  return launch_kernel(k, ca, grid, FAST_BD, shm, st, e0, e1);
}

hipError_t launch_fast_batch(const FastArgs& a, uint32_t n, const BatchArgs& b, uint32_t grid, size_t shm,
                             hipStream_t st, hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn(n, FAST_PLAIN, PIN_BATCH);
  const uint64_t units = (uint64_t)b.n_sets * b.slices;
  if (!k || !b.sets || !units || b.slices > BATCH_MAX_SLICES || !b.runlen || grid > units)
    return hipErrorInvalidValue;
  BatchFastArgs ba{};
  static_cast<FastArgs&>(ba) = a;
  ba.bz = b;
  return launch_kernel(k, ba, grid, FAST_BD, shm, st, e0, e1);
}
#endif  // BOTE_FAST_CON_UNIT

}  // namespace bote
