// bote_sweep.hip — the fast-path sweep kernel (gfx950): exhaustive search over
// colex ranks with a block top-K, for planets that meet the fast-path
// preconditions checked on the host (bote_capi_sweep.hip, fast_eligible):
//   * every latency <= 4095 (packed u16 keys: latency << 4 | member)
//   * the server set is "simple": self latency 0, latency between two servers
//     > 0 (a colocated client's nearest server is itself)
//   * servers in name order, >= 2 clients, min_fairness_fpaxos_improv == 0
// Anything else runs the generic kernel (bote_kernels.hip), which is also the
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
// Per config (one lane; reference functions in bote_kernels.hip's header):
// quorum latencies by sorting each member's off-diagonal distances; FPaxos
// leader by exact-COV comparison (variance is shift invariant, so leader l's
// V = nc*sum(L^2) - (sum L)^2 of its column, precomputed per position); the
// Input leaderless keys by the packed client-quad loop; compute_score validity
// by integer / f64-margin decisions; digest; block top-K.
#include "bote_fast.hpp"
#include <type_traits>

#include "bote_launch.hpp"
#include "bote_pinned.hpp"


namespace bote {


constexpr uint32_t QSH = 10;  // log2(FAST_BD * 4): byte stride between qtab member planes
static_assert((1u << QSH) == FAST_BD * 4, "qtab plane stride");

struct FastSmem {
  unsigned char* base;  // dynamic LDS base; byte offsets below are relative to it
  uint32_t cqt, rqt, qtab;
  uint32_t* srv;
  uint32_t* cs1;
  uint64_t* cs2;
  double* vcol;
  uint64_t* binom;
  uint32_t* cmax;  // FAST_MAX: per position, the largest client latency of its column
  uint2* c4;       // FAST_LIST: per position, its column's four largest client latencies, descending (4 x u16)
  uint64_t* ch;    // FAST_MDTM: per position, H of its client column (mdtm_key; shift invariant, so also H of ff1 and ff2)
  TopkLds tk;
};

__host__ __device__ inline size_t fast_layout(const FastArgs& a, int N, int NLW, int tail, size_t* off) {
  size_t o = 0;
  off[0] = o; o += (size_t)N * FAST_BD * NLW * 4;  // qtab first: offsets stay small
  off[1] = o; o += (size_t)a.R * a.cq_stride * 8;
  off[2] = o; o += a.rq_separate ? (size_t)a.R * a.rq_stride * 8 : 0;
  off[3] = o; o += (size_t)a.ns * 4;  // srv
  off[4] = o; o += (size_t)a.ns * 4;  // cs1
  o = (o + 15) & ~(size_t)15;
  off[5] = o; o += (size_t)a.ns * 8;                   // cs2
  off[6] = o; o += (size_t)a.ns * 8;                   // vcol
  off[7] = o; o += (size_t)(a.ns + 1) * (N + 1) * 8;  // binom
  o = (o + 15) & ~(size_t)15;
  off[8] = o; o += (size_t)a.n_obj * KP * 16;  // top
  off[9] = o; o += (size_t)FAST_BD * 16;      // cand
  off[10] = o; o += (size_t)KP * 16;          // tmp
  off[11] = o; o += (size_t)MAXOBJ * 16;      // thr
  off[12] = o; o += 48;                       // cnt[1 + MAXOBJ]
  off[13] = o; o += tail == FAST_MAX ? (size_t)a.ns * 4 : 0;   // cmax
  off[14] = o; o += tail == FAST_LIST ? (size_t)a.ns * 8 : 0;  // c4 (8-byte aligned: every region above is)
  off[15] = o; o += tail == FAST_MDTM ? (size_t)a.ns * 8 : 0;  // ch (the same)
  return o;
}

size_t fast_smem_bytes(const FastArgs& a, uint32_t n, int tail) {
  size_t off[16];
  int nl = 0;
  switch (n) {
#define NL_CASE(NN) case NN: nl = QCfg<NN>::NL; break;
    NL_CASE(2) NL_CASE(3) NL_CASE(4) NL_CASE(5) NL_CASE(6) NL_CASE(7) NL_CASE(8) NL_CASE(9)
    NL_CASE(10) NL_CASE(11) NL_CASE(12) NL_CASE(13) NL_CASE(14) NL_CASE(15) NL_CASE(16)
#undef NL_CASE
    default: return 0;
  }
  return fast_layout(a, (int)n, nl <= 2 ? 1 : 2, tail, off);
}

template <int N>
__device__ __forceinline__ uint32_t sel_u(const uint32_t (&arr)[N], uint32_t i) {
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) r |= arr[j] & (0u - (uint32_t)(i == (uint32_t)j));
  return r;
}


// ------------------------------------------------- sorted lists (LIST) ----
// A slot's four largest values, descending, as 4 x u16 in two words (the fast
// path's values are at most 2 * 4095): l[0] = v0 | v1 << 16, l[1] = v2 | v3 << 16.
static_assert(PCTL_FAST_DEPTH == 4, "the packed lists and their merge are four deep");
__device__ __forceinline__ void sort_desc(uint32_t& hi, uint32_t& lo) {
  const uint32_t h = max(hi, lo);
  lo = min(hi, lo);
  hi = h;
}
// insert v into the descending list l (each 16-bit half its own list); the least drops out
__device__ __forceinline__ void pk_insert(us2 (&l)[PCTL_FAST_DEPTH], us2 v) {
#pragma unroll
  for (int i = 0; i < PCTL_FAST_DEPTH; ++i) {
    const us2 hi = __builtin_elementwise_max(l[i], v);
    if (i + 1 < PCTL_FAST_DEPTH) v = __builtin_elementwise_min(l[i], v);
    l[i] = hi;
  }
}
__device__ __forceinline__ void list_insert(uint32_t (&l)[PCTL_FAST_DEPTH], uint32_t v) {
#pragma unroll
  for (int i = 0; i < PCTL_FAST_DEPTH; ++i) {
    const uint32_t hi = max(l[i], v);
    if (i + 1 < PCTL_FAST_DEPTH) v = min(l[i], v);
    l[i] = hi;
  }
}
// the k-th largest (k = 1..4, uniform) of a packed list
__device__ __forceinline__ uint32_t list_at(const uint32_t (&l)[2], uint32_t k) {
  const uint32_t w = k > 2 ? l[1] : l[0];
  return (k & 1) ? (w & 0xFFFFu) : (w >> 16);
}

// ------------------------------------------------------------ hot loop ----
// Input leaderless keys over client quads.  Per quad and member: one
// ds_read_b64 (4 clients), a packed OR of the member index and a packed min
// (v_pk_min_u16: ties go to the lower member = the lower name); per client:
// one qtab read for the nearest member's quorum latencies; packed adds and
// v_dot2_u32_u16 accumulate the sum and the sum of squares.  Squares are
// accumulated in 32 bits and flushed to 64 bits every `flushQ` quads.
// TAIL == FAST_MAX: also each table's largest client latency into MX, one packed max
// (v_pk_max_u16) per half quad into a running register per table, taken after
// the remainder mask (a dead client counts 0); no LDS traffic is added.
// TAIL == FAST_LIST: each table's four largest client latencies into ML,
// descending, as 4 x u16 in two words.  The loop keeps, per table, a descending
// list of four packed registers: the low halves are one stream (clients 0 and
// 2 of every quad), the high halves another (clients 1 and 3), and a masked
// half quad is inserted into both at once by 7 packed compare-exchange steps
// (v_pk_max_u16 / v_pk_min_u16).  After the loop the two streams' lists are
// merged.  A dead client enters as 0 and cannot displace a live value among
// the largest `need <= nc`.  No LDS traffic is added here either.
// TAIL == FAST_MDTM: H of the tables in the mask `mdm` (bit t: table t has an
// MDTM objective; uniform over the launch) into MH.  A table's mean is known
// only after the loop, so the quads are passed over a second time: the same
// loads, packed nearest-member min, qtab reads and remainder mask, then per
// table in the mask a packed saturating subtract of T = floor(S1 / nc)
// (v_pk_sub_u16 clamp), whose sum (v_dot2_u32_u16) is A = the sum of max(x - T,
// 0) and whose non-zero halves (v_pk_min_u16 with 1, v_dot2_u32_u16) count B =
// the number of x > T; H = nc A - r B (bote_device.hpp mdtm_h).  A dead
// remainder client is masked to 0 before the subtract and adds nothing to
// either.  x <= 2 * 4095 and nc <= 4096, so A <= 2^25 and B <= 2^12 stay in 32
// bits for the whole loop.  Tables outside the mask, and a launch with an
// empty mask, pay nothing.
template <int N, int NL, int TAIL>
__device__ __forceinline__ void client_quads(const unsigned char* B, uint32_t cqt, uint32_t nq, uint32_t rem,
                                             uint32_t flushQ, const uint32_t (&colT)[N], uint32_t qlane,
                                             uint32_t (&S1)[NL], uint64_t (&S2)[NL], uint32_t (&MX)[NL],
                                             uint32_t (&ML)[NL][2], uint32_t mdm, uint32_t nc, uint64_t (&MH)[NL]) {
  const us2 ones = {1, 1};
  constexpr int NQ = NL == 3 ? 8 : 4;  // qtab words per quad
  uint32_t s2[NL];
  us2 pm[NL];  // FAST_MAX: running packed maxima
  us2 pl[NL][PCTL_FAST_DEPTH];  // FAST_LIST: running packed lists, descending
#pragma unroll
  for (int t = 0; t < NL; ++t) {
    S1[t] = 0;
    S2[t] = 0;
    s2[t] = 0;
    if constexpr (TAIL == FAST_MAX) pm[t] = us2{0, 0};
    if constexpr (TAIL == FAST_LIST) {
#pragma unroll
      for (int i = 0; i < PCTL_FAST_DEPTH; ++i) pl[t][i] = us2{0, 0};
    }
  }
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
  // `plane2`: the third table's plane too (the second pass of FAST_MDTM skips it
  // when that table has no MDTM objective)
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
  auto acc1 = [&](int t, us2 dlo, us2 dhi, uint32_t ql01, uint32_t ql23, uint32_t mlo, uint32_t mhi) {
    us2 a01 = dlo + as_us2(ql01), a23 = dhi + as_us2(ql23);
    a01 = as_us2(as_u32(a01) & mlo);
    a23 = as_us2(as_u32(a23) & mhi);
    S1[t] = __builtin_amdgcn_udot2(a01, ones, S1[t], false);
    S1[t] = __builtin_amdgcn_udot2(a23, ones, S1[t], false);
    s2[t] = __builtin_amdgcn_udot2(a01, a01, s2[t], false);
    s2[t] = __builtin_amdgcn_udot2(a23, a23, s2[t], false);
    if constexpr (TAIL == FAST_MAX) pm[t] = __builtin_elementwise_max(__builtin_elementwise_max(pm[t], a01), a23);
    if constexpr (TAIL == FAST_LIST) {
      pk_insert(pl[t], a01);
      pk_insert(pl[t], a23);
    }
  };
  auto accum = [&](us2 lo, us2 hi, const uint32_t (&q)[NQ], uint32_t mlo, uint32_t mhi) {
    const us2 dlo = lo >> (us2)4, dhi = hi >> (us2)4;
    acc1(0, dlo, dhi, __builtin_amdgcn_perm(q[1], q[0], 0x05040100u), __builtin_amdgcn_perm(q[3], q[2], 0x05040100u),
         mlo, mhi);
    if (NL >= 2)
      acc1(NL >= 2 ? 1 : 0, dlo, dhi, __builtin_amdgcn_perm(q[1], q[0], 0x07060302u),
           __builtin_amdgcn_perm(q[3], q[2], 0x07060302u), mlo, mhi);
    if (NL == 3)
      acc1(NL - 1, dlo, dhi, __builtin_amdgcn_perm(q[NQ - 3], q[NQ - 4], 0x05040100u),
           __builtin_amdgcn_perm(q[NQ - 1], q[NQ - 2], 0x05040100u), mlo, mhi);
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
    const uint32_t mlo = rem >= 2 ? ~0u : 0x0000FFFFu, mhi = rem == 3 ? 0x0000FFFFu : 0u;
    quad(nq * 8, mlo, mhi);
    flush();
  }
  if constexpr (TAIL == FAST_MAX) {
#pragma unroll
    for (int t = 0; t < NL; ++t) MX[t] = max((uint32_t)pm[t].x, (uint32_t)pm[t].y);
  }
  if constexpr (TAIL == FAST_LIST) {
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      // the four largest of two descending lists A and B: max(A[i], B[3 - i])
      // holds them as a bitonic sequence, which two exchange stages sort
      uint32_t c[PCTL_FAST_DEPTH];
#pragma unroll
      for (int i = 0; i < PCTL_FAST_DEPTH; ++i) c[i] = max((uint32_t)pl[t][i].x, (uint32_t)pl[t][PCTL_FAST_DEPTH - 1 - i].y);
      sort_desc(c[0], c[2]);
      sort_desc(c[1], c[3]);
      sort_desc(c[0], c[1]);
      sort_desc(c[2], c[3]);
      ML[t][0] = c[0] | (c[1] << 16);
      ML[t][1] = c[2] | (c[3] << 16);
    }
  }
  if constexpr (TAIL == FAST_MDTM) {
#pragma unroll
    for (int t = 0; t < NL; ++t) MH[t] = 0;
    if (mdm) {
      MdtmThr thr[NL];
      us2 pT[NL];  // T in both halves (T <= 2 * 4095)
      uint32_t A[NL], C[NL];
#pragma unroll
      for (int t = 0; t < NL; ++t) {
        thr[t] = (mdm >> t) & 1u ? mdtm_thr(S1[t], nc) : MdtmThr{0, 0};  // (uniform: no division for the others)
        pT[t] = us2{(unsigned short)thr[t].T, (unsigned short)thr[t].T};
        A[t] = C[t] = 0;
      }
      auto above1 = [&](int t, us2 dlo, us2 dhi, uint32_t ql01, uint32_t ql23, uint32_t mlo, uint32_t mhi) {
        if (!(mdm & (1u << t))) return;  // uniform
        const us2 a01 = as_us2(as_u32(dlo + as_us2(ql01)) & mlo), a23 = as_us2(as_u32(dhi + as_us2(ql23)) & mhi);
        const us2 e01 = __builtin_elementwise_sub_sat(a01, pT[t]), e23 = __builtin_elementwise_sub_sat(a23, pT[t]);
        A[t] = __builtin_amdgcn_udot2(e01, ones, A[t], false);
        A[t] = __builtin_amdgcn_udot2(e23, ones, A[t], false);
        C[t] = __builtin_amdgcn_udot2(__builtin_elementwise_min(e01, ones), ones, C[t], false);
        C[t] = __builtin_amdgcn_udot2(__builtin_elementwise_min(e23, ones), ones, C[t], false);
      };
      auto quad2 = [&](uint32_t g8, uint32_t mlo, uint32_t mhi) {
        uint2 w[N];
        uint32_t q[NQ] = {};
        us2 lo, hi;
        load(g8, w);
        nearest(w, lo, hi);
        qread(lo, hi, q, (mdm >> 2) & 1u);  // (uniform)
        const us2 dlo = lo >> (us2)4, dhi = hi >> (us2)4;
        above1(0, dlo, dhi, __builtin_amdgcn_perm(q[1], q[0], 0x05040100u),
               __builtin_amdgcn_perm(q[3], q[2], 0x05040100u), mlo, mhi);
        if (NL >= 2)
          above1(NL >= 2 ? 1 : 0, dlo, dhi, __builtin_amdgcn_perm(q[1], q[0], 0x07060302u),
                 __builtin_amdgcn_perm(q[3], q[2], 0x07060302u), mlo, mhi);
        if (NL == 3)
          above1(NL - 1, dlo, dhi, __builtin_amdgcn_perm(q[NQ - 3], q[NQ - 4], 0x05040100u),
                 __builtin_amdgcn_perm(q[NQ - 1], q[NQ - 2], 0x05040100u), mlo, mhi);
      };
      for (uint32_t g2 = 0; g2 < nq; ++g2) quad2(g2 * 8, ~0u, ~0u);
      if (rem) quad2(nq * 8, rem >= 2 ? ~0u : 0x0000FFFFu, rem == 3 ? 0x0000FFFFu : 0u);
#pragma unroll
      for (int t = 0; t < NL; ++t) MH[t] = mdtm_h(nc, thr[t], A[t], C[t]);
    }
  }
}

// FAST_MDTM: H (mdtm_key) of n values x[0..n) with sum s1, a two-step
// computation in registers (the colocated slots: n <= 16 members)
template <int N>
__device__ __forceinline__ uint64_t small_mdtm_h(const uint32_t (&x)[N], uint32_t s1) {
  const MdtmThr t = mdtm_thr(s1, (uint32_t)N);
  uint32_t A = 0, C = 0;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    A += x[k] > t.T ? x[k] - t.T : 0u;
    C += x[k] > t.T ? 1u : 0u;
  }
  return mdtm_h((uint32_t)N, t, A, C);
}

// ---------------------------------------------------------- the kernel ----
// TAIL == FAST_MAX: the variant for sweeps with a MAX objective (base key set).  It also
// carries each slot's maximum: the Input leaderless tables' from the client
// loop, Input FPaxos in closed form (the leader column's largest latency,
// staged per position beside cs1/cs2, plus the quorum latency), and the
// colocated slots' from the values the Q phase and the N-step loop already
// hold.  The MAX keys are built just before finish_config, which leaves them
// alone, and withdrawn when it defers the config: built after it, the ten
// maxima stay live across the score and digest arithmetic and N = 7 spills
// (8 B/lane of scratch; none this way).
// TAIL == FAST_LIST: the variant for sweeps with a percentile objective that
// needs at most four of its slot's largest values (base key set).  It carries
// each slot's four largest values, descending, where FAST_MAX carries the
// largest: the Input leaderless tables' from the client loop's packed lists,
// Input FPaxos from the leader column's four largest latencies (staged per
// position, c4) plus the quorum latency, the colocated leaderless from the
// lane's quorum table read back after the client loop (nothing more is live
// across it), colocated FPaxos from the N-step loop.  Entry 0 is the maximum,
// so the MAX objectives of such a sweep are served from the lists.  Keys are
// built and withdrawn as for FAST_MAX.
// TAIL == FAST_MDTM: the variant for sweeps with an MDTM objective and no MAX
// or percentile one (base key set).  Only the slots that have an MDTM
// objective are treated (a mask over the launch, from obj_kind / obj_slot):
// the Input leaderless tables by client_quads' second pass; Input FPaxos from
// H of the leader's client column (staged per position, ch: H is shift
// invariant, the quorum latency drops out); the colocated leaderless slots
// from the lane's quorum table read back, colocated FPaxos from the N-step
// loop's values again, both in registers (small_mdtm_h).  Each H goes into its
// objectives' keys at once, before finish_config, which leaves them alone;
// they are withdrawn when it defers the config.
// PIN: the pinned variant (bote_pinned.hpp; FAST_PLAIN only).  [rb, re) are
// pinned ranks; a lane walks `runlen` of them over the free indices q and
// re-merges the members per step.  The full colex rank is computed with the
// members, always: the digest, a record offered to the top-K and a deferred
// config's queue entry carry it, and everything after p[N] is the code of the
// unpinned kernel.
template <int N, int TAIL, bool PIN = false>
__global__ void __launch_bounds__(FAST_BD, 4) sweep_fast_kernel(std::conditional_t<PIN, PinFastArgs, FastArgs> a) {
  static_assert(!PIN || TAIL == FAST_PLAIN, "the pinned variant computes SCORE, MEAN and COV objectives");
  using QC = QCfg<N>;
  constexpr int NL = QC::NL;
  constexpr int NLW = NL <= 2 ? 1 : 2;
  constexpr int P = Pow2<N - 1>::v;  // off-diagonal row values, padded
  extern __shared__ __align__(16) unsigned char smem[];
  size_t off[16];
  fast_layout(a, N, NLW, TAIL, off);
  FastSmem s;
  s.base = smem;
  s.qtab = (uint32_t)off[0];
  s.cqt = (uint32_t)off[1];
  s.rqt = a.rq_separate ? (uint32_t)off[2] : (uint32_t)off[1];
  s.srv = (uint32_t*)(smem + off[3]);
  s.cs1 = (uint32_t*)(smem + off[4]);
  s.cs2 = (uint64_t*)(smem + off[5]);
  s.vcol = (double*)(smem + off[6]);
  s.binom = (uint64_t*)(smem + off[7]);
  s.cmax = (uint32_t*)(smem + off[13]);
  s.c4 = (uint2*)(smem + off[14]);
  s.ch = (uint64_t*)(smem + off[15]);
  s.tk.top = (Rec*)(smem + off[8]);
  s.tk.cand = (Rec*)(smem + off[9]);
  s.tk.tmp = (Rec*)(smem + off[10]);
  s.tk.thr = (Rec*)(smem + off[11]);
  s.tk.cnt = (int*)(smem + off[12]);
  const uint32_t tid = threadIdx.x;
  const unsigned char* B = smem;

  // ---- stage: quad matrices, server list, binomials; then per-position sums
  {
    const uint32_t cw = a.R * a.cq_stride * 2;  // 32-bit words
    const uint32_t* src = (const uint32_t*)a.cqt;
    uint32_t* dst = (uint32_t*)(smem + s.cqt);
    for (uint32_t i = tid; i < cw; i += FAST_BD) dst[i] = src[i];
    if (a.rq_separate) {
      const uint32_t rw = a.R * a.rq_stride * 2;
      const uint32_t* rs = (const uint32_t*)a.rqt;
      uint32_t* rd = (uint32_t*)(smem + s.rqt);
      for (uint32_t i = tid; i < rw; i += FAST_BD) rd[i] = rs[i];
    }
  }
  for (uint32_t i = tid; i < a.ns; i += FAST_BD) s.srv[i] = a.srv[i];
  for (uint32_t i = tid; i < (a.ns + 1) * (N + 1); i += FAST_BD) s.binom[i] = a.binom[i];
  topk_init(s.tk, a.n_obj);
  __syncthreads();
  const uint32_t cstride = a.cq_stride * 8;  // bytes per CQT column
  const uint32_t rstride = a.rq_stride * 8;
  for (uint32_t i = tid; i < a.ns; i += FAST_BD) {
    const uint32_t col = s.cqt + s.srv[i] * cstride;
    uint64_t c1 = 0, c2 = 0;
    uint32_t cm = 0;
    for (uint32_t c = 0; c < a.nc; ++c) {
      uint64_t v = ld16(B, col + (c >> 2) * 8 + (c & 3) * 2) >> LAT_SHIFT;
      c1 += v;
      c2 += v * v;
      if constexpr (TAIL == FAST_MAX) cm = max(cm, (uint32_t)v);
    }
    if constexpr (TAIL == FAST_MAX) s.cmax[i] = cm;
    if constexpr (TAIL == FAST_LIST) {  // (a pass of its own: once per block)
      uint32_t cl[PCTL_FAST_DEPTH] = {0, 0, 0, 0};
      for (uint32_t c = 0; c < a.nc; ++c) list_insert(cl, ld16(B, col + (c >> 2) * 8 + (c & 3) * 2) >> LAT_SHIFT);
      s.c4[i] = make_uint2(cl[0] | (cl[1] << 16), cl[2] | (cl[3] << 16));
    }
    if constexpr (TAIL == FAST_MDTM) {  // (a pass of its own: once per block)
      const MdtmThr t = mdtm_thr((uint32_t)c1, a.nc);
      uint32_t A = 0, C = 0;
      for (uint32_t c = 0; c < a.nc; ++c) {
        const uint32_t v = ld16(B, col + (c >> 2) * 8 + (c & 3) * 2) >> LAT_SHIFT;
        A += v > t.T ? v - t.T : 0u;
        C += v > t.T ? 1u : 0u;
      }
      s.ch[i] = mdtm_h(a.nc, t, A, C);
    }
    s.cs1[i] = (uint32_t)c1;
    s.cs2[i] = c2;
    s.vcol[i] = (double)((uint64_t)a.nc * c2 - c1 * c1);  // exact: < 2^53
  }
  __syncthreads();

  const uint32_t nc = a.nc, nq = nc >> 2, rem = nc & 3;
  const uint32_t qlane = s.qtab + tid * 4;
  const uint64_t total = a.re - a.rb;
  const uint64_t runlen = a.runlen;
  const uint64_t njobs = (total + runlen - 1) / runlen;
  const uint64_t G = (uint64_t)gridDim.x * FAST_BD;
  const uint64_t outer = (njobs + G - 1) / G;
  const double pnc1 = a.p_fmean * (double)nc, pnc2 = a.p_emean * (double)nc;
  uint64_t valid_cnt = 0, digest = 0;
  // FAST_MDTM: the slots (bit = slot) and the leaderless tables (bit = table)
  // that have an MDTM objective
  uint32_t mds = 0, mdm = 0;
  if constexpr (TAIL == FAST_MDTM) {
    for (int o = 0; o < a.n_obj; ++o)
      if (a.obj_kind[o] == OBJ_MDTM) mds |= 1u << a.obj_slot[o];
    mdm = ((mds >> SLOT_AF1) & 1u) << QC::idx_a1 | ((mds >> SLOT_AF2) & 1u) << QC::idx_a2 |
          ((mds >> SLOT_E) & 1u) << QC::idx_e;
  }

  for (uint64_t it = 0; it < outer; ++it) {
    const uint64_t job = it * G + (uint64_t)blockIdx.x * FAST_BD + tid;
    const bool jobok = job < njobs;
    uint64_t rank = a.rb + job * runlen;
    uint32_t p[N];
#pragma unroll
    for (int j = 0; j < N; ++j) p[j] = j;
    [[maybe_unused]] uint32_t q[PIN ? N : 1];  // PIN: the free indices (one unused word otherwise)
    if constexpr (PIN) {
#pragma unroll
      for (int j = 0; j < N; ++j) q[j] = 0;
      if (jobok) pin_unrank<N>(s.binom, a.ns, a.pz, rank, q);
    } else {
      if (jobok) colex_unrank<N>(s.binom, a.ns, rank, p);
    }
    for (uint64_t tt = 0; tt < runlen; ++tt) {
      bool have = jobok && rank < a.re;
      uint64_t frank = rank;  // the config's full colex rank (PIN: `rank` is the pinned rank)
      if constexpr (PIN) {
        if (have) pin_members<N>(s.binom, a.pz, q, p, frank);
      }
      uint64_t key[MAXOBJ];
      bool ok[MAXOBJ];
#pragma unroll
      for (int o = 0; o < MAXOBJ; ++o) {
        key[o] = 0;
        ok[o] = false;
      }
      if (have) {
        // ---- members (positions ascending == names ascending)
        uint32_t colT[N], colR[N], rowq[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const uint32_t r = a.srv_identity ? p[j] : s.srv[p[j]];
          colT[j] = r * cstride;
          colR[j] = s.rqt + r * rstride;
          rowq[j] = (r >> 2) * 8 + (r & 3) * 2;
        }
        // ---- Q phase: sorted off-diagonal distances of each member's row
        uint32_t Q2[N], Q3[N];
        uint32_t cS1[NL], cS2[NL];
        uint32_t cMX[NL];  // FAST_MAX: the colocated leaderless maxima
#pragma unroll
        for (int t = 0; t < NL; ++t) cS1[t] = cS2[t] = cMX[t] = 0;
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
            if constexpr (TAIL == FAST_MAX) cMX[t2] = max(cMX[t2], ql[t2]);
          }
          *(uint32_t*)(smem + qlane + ((uint32_t)j << QSH)) = ql[0] | (NL >= 2 ? ql[NL >= 2 ? 1 : 0] << 16 : 0u);
          if (NL == 3) *(uint32_t*)(smem + qlane + ((uint32_t)(N + j) << QSH)) = ql[NL - 1];
          // one member row at a time: keeps the row's reads and sort network
          // from being interleaved with the next rows (register pressure)
          __builtin_amdgcn_sched_barrier(0);
        }
        // ---- FPaxos leader (f = 1, q = 2, min COV, first in config order)
        uint32_t bi = 0;
        bool amb = false;
        // the leader's position, quorum latencies and column, carried along
        uint32_t lp = p[0], lq2 = Q2[0], lq3 = Q3[0], lcol = colR[0];
        {
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
              bi = l;
              bS = S;
              bV = V;
              lp = p[l];
              lq2 = Q2[l];
              lq3 = Q3[l];
              lcol = colR[l];
            }
          }
        }
        if (amb) {  // defer to the exact generic kernel (see bote_sweep_launch)
          defer_rank(a, frank);
          have = false;
        }
        if (have) {
          Mom mom[NSLOT];
          uint32_t mx[NSLOT];     // FAST_MAX: the slots' maxima
          uint32_t l4[NSLOT][2];  // FAST_LIST: the slots' four largest values, packed (FPaxos: less the quorum latency)
          // FAST_MDTM: slot q's H into the keys of its MDTM objectives (`q` is
          // a constant and the objectives uniform: scalar branches)
          auto mdtm_keys = [&](int q, uint64_t h) {
#pragma unroll
            for (int o = 0; o < MAXOBJ; ++o) {
              if (o >= a.n_obj) break;
              if (a.obj_kind[o] != OBJ_MDTM || a.obj_slot[o] != (uint32_t)q) continue;
              ok[o] = true;
              key[o] = mdtm_key(h, mom[q].s1);
            }
          };
          // Input leaderless: the hot loop (first, so little is live across it)
          {
            uint32_t S1[NL];
            uint64_t S2[NL];
            uint32_t MX[NL];
            uint32_t ML[NL][2];
            uint64_t MH[NL];
            client_quads<N, NL, TAIL>(B, s.cqt, ABLATE(a, 1) ? 0u : nq, ABLATE(a, 1) ? 0u : rem, a.s2_flush, colT,
                                      qlane, S1, S2, MX, ML, mdm, nc, MH);
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
            if constexpr (TAIL == FAST_MAX) {
              mx[SLOT_AF1] = MX[QC::idx_a1];
              mx[SLOT_AF2] = MX[QC::idx_a2];
              mx[SLOT_E] = MX[QC::idx_e];
            }
            if constexpr (TAIL == FAST_LIST) {
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                l4[SLOT_AF1][h] = ML[QC::idx_a1][h];
                l4[SLOT_AF2][h] = ML[QC::idx_a2][h];
                l4[SLOT_E][h] = ML[QC::idx_e][h];
              }
            }
            if constexpr (TAIL == FAST_MDTM) {
              if ((mds >> SLOT_AF1) & 1u) mdtm_keys(SLOT_AF1, MH[QC::idx_a1]);
              if ((mds >> SLOT_AF2) & 1u) mdtm_keys(SLOT_AF2, MH[QC::idx_a2]);
              if ((mds >> SLOT_E) & 1u) mdtm_keys(SLOT_E, MH[QC::idx_e]);
            }
          }
          // Input FPaxos: moments from the leader column's sums
          mom[SLOT_FF1] = leader_mom(s.cs1[lp], s.cs2[lp], nc, lq2);
          mom[SLOT_FF2] = leader_mom(s.cs1[lp], s.cs2[lp], nc, lq3);
          if constexpr (TAIL == FAST_MAX) {
            const uint32_t cm = s.cmax[lp];
            mx[SLOT_FF1] = cm + lq2;
            mx[SLOT_FF2] = cm + lq3;
          }
          if constexpr (TAIL == FAST_LIST) {
            const uint2 c = s.c4[lp];
            l4[SLOT_FF1][0] = l4[SLOT_FF2][0] = c.x;
            l4[SLOT_FF1][1] = l4[SLOT_FF2][1] = c.y;
          }
          if constexpr (TAIL == FAST_MDTM) {
            if ((mds >> SLOT_FF1) & 1u) mdtm_keys(SLOT_FF1, s.ch[lp]);
            if ((mds >> SLOT_FF2) & 1u) mdtm_keys(SLOT_FF2, s.ch[lp]);
          }
          // Colocated: leaderless values are the members' own quorum latencies;
          // FPaxos reads the leader's column of the config submatrix.
          {
            uint32_t f1 = 0, f1s = 0, f2 = 0, f2s = 0;
            uint32_t fm = 0;  // FAST_MAX: the members' largest latency to the leader
#pragma unroll
            for (int k = 0; k < N; ++k) {
              const uint32_t v = ld16(B, lcol + rowq[k]) >> LAT_SHIFT;
              if constexpr (TAIL == FAST_MAX) fm = max(fm, v);
              const uint32_t x1 = v + lq2, x2 = v + lq3;
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
            if constexpr (TAIL == FAST_MAX) {
              mx[5 + SLOT_FF1] = fm + lq2;
              mx[5 + SLOT_FF2] = fm + lq3;
              mx[5 + SLOT_AF1] = cMX[QC::idx_a1];
              mx[5 + SLOT_AF2] = cMX[QC::idx_a2];
              mx[5 + SLOT_E] = cMX[QC::idx_e];
            }
            if constexpr (TAIL == FAST_LIST) {
              // the members' four largest latencies to the leader (the N-step loop's values again)
              uint32_t fl[PCTL_FAST_DEPTH] = {0, 0, 0, 0};
#pragma unroll
              for (int k = 0; k < N; ++k) list_insert(fl, ld16(B, lcol + rowq[k]) >> LAT_SHIFT);
              l4[5 + SLOT_FF1][0] = l4[5 + SLOT_FF2][0] = fl[0] | (fl[1] << 16);
              l4[5 + SLOT_FF1][1] = l4[5 + SLOT_FF2][1] = fl[2] | (fl[3] << 16);
              // the members' own quorum latencies, read back from the lane's
              // qtab planes: word j holds tables 0 and 1, word N + j table 2
              us2 pa[PCTL_FAST_DEPTH], pb[PCTL_FAST_DEPTH];
#pragma unroll
              for (int i = 0; i < PCTL_FAST_DEPTH; ++i) pa[i] = pb[i] = us2{0, 0};
#pragma unroll
              for (int j = 0; j < N; ++j) {
                pk_insert(pa, as_us2(ld32(B, qlane + ((uint32_t)j << QSH))));
                if (NL == 3) pk_insert(pb, as_us2(ld32(B, qlane + ((uint32_t)(N + j) << QSH))));
              }
              uint32_t cl[3][2];
#pragma unroll
              for (int h = 0; h < 2; ++h) {
                cl[0][h] = (uint32_t)pa[2 * h].x | ((uint32_t)pa[2 * h + 1].x << 16);
                cl[1][h] = (uint32_t)pa[2 * h].y | ((uint32_t)pa[2 * h + 1].y << 16);
                cl[2][h] = (uint32_t)pb[2 * h].x | ((uint32_t)pb[2 * h + 1].x << 16);
                l4[5 + SLOT_AF1][h] = cl[QC::idx_a1][h];
                l4[5 + SLOT_AF2][h] = cl[QC::idx_a2][h];
                l4[5 + SLOT_E][h] = cl[QC::idx_e][h];
              }
            }
            if constexpr (TAIL == FAST_MDTM) {
              if (((mds >> (5 + SLOT_FF1)) | (mds >> (5 + SLOT_FF2))) & 1u) {
                // the members' latencies to the leader (the N-step loop's values
                // again; the quorum latency drops out of H)
                uint32_t x[N];
#pragma unroll
                for (int k = 0; k < N; ++k) x[k] = ld16(B, lcol + rowq[k]) >> LAT_SHIFT;
                const uint64_t h = small_mdtm_h<N>(x, f1 - (uint32_t)N * lq2);
                if ((mds >> (5 + SLOT_FF1)) & 1u) mdtm_keys(5 + SLOT_FF1, h);
                if ((mds >> (5 + SLOT_FF2)) & 1u) mdtm_keys(5 + SLOT_FF2, h);
              }
              // the members' own quorum latencies, read back from the lane's
              // qtab planes: word j holds tables 0 and 1, word N + j table 2
#pragma unroll
              for (int t = 0; t < NL; ++t) {
                const uint32_t want = ((mds >> (5 + SLOT_AF1)) & 1u) << QC::idx_a1 |
                                      ((mds >> (5 + SLOT_AF2)) & 1u) << QC::idx_a2 |
                                      ((mds >> (5 + SLOT_E)) & 1u) << QC::idx_e;
                if (!((want >> t) & 1u)) continue;
                uint32_t x[N];
#pragma unroll
                for (int j = 0; j < N; ++j) {
                  const uint32_t w = ld32(B, qlane + ((uint32_t)(t == 2 ? N + j : j) << QSH));
                  x[j] = t == 1 ? w >> 16 : w & 0xFFFFu;
                }
                const uint64_t h = small_mdtm_h<N>(x, cS1[t]);
                if (QC::idx_a1 == t && ((mds >> (5 + SLOT_AF1)) & 1u)) mdtm_keys(5 + SLOT_AF1, h);
                if (QC::idx_a2 == t && ((mds >> (5 + SLOT_AF2)) & 1u)) mdtm_keys(5 + SLOT_AF2, h);
                if (QC::idx_e == t && ((mds >> (5 + SLOT_E)) & 1u)) mdtm_keys(5 + SLOT_E, h);
              }
            }
          }
          if constexpr (TAIL == FAST_LIST) {
            // the MAX and percentile keys first, as below for FAST_MAX
#pragma unroll
            for (int o = 0; o < MAXOBJ; ++o) {
              if (o >= a.n_obj) break;
              const uint32_t kind = a.obj_kind[o];
              if (kind < OBJ_MAX) continue;
              const uint32_t sl = a.obj_slot[o];
              const bool pctl = kind >= OBJ_PCTL;
              const uint32_t need = pctl ? kind & PCTL_NEED_MASK : 1u;  // (MAX: the first entry)
              const bool whole = pctl && (kind & PCTL_WHOLE);
#pragma unroll
              for (int q = 0; q < NSLOT; ++q) {
                if ((uint32_t)q != sl) continue;
                const uint32_t add = q % 5 == SLOT_FF1 ? lq2 : q % 5 == SLOT_FF2 ? lq3 : 0u;
                const uint32_t v = list_at(l4[q], need) + add;
                const uint32_t twice = whole ? v + list_at(l4[q], need - 1) + add : 2 * v;
                ok[o] = true;
                key[o] = pctl ? pctl_key(twice, mom[q].s1) : max_key(v, mom[q].s1);
              }
            }
          }
          if constexpr (TAIL == FAST_MAX) {
            // the MAX keys first (the maxima die here, before the score and
            // digest arithmetic); a deferred config withdraws them below
#pragma unroll
            for (int o = 0; o < MAXOBJ; ++o) {
              if (o >= a.n_obj) break;
              if (a.obj_kind[o] != OBJ_MAX) continue;
              const uint32_t sl = a.obj_slot[o];
              // `sl` is uniform: one scalar branch per slot
#pragma unroll
              for (int q = 0; q < NSLOT; ++q) {
                if ((uint32_t)q != sl) continue;
                ok[o] = true;
                key[o] = max_key(mx[q], mom[q].s1);
              }
            }
          }
          if (!finish_config<N, TAIL>(a, mom, s.vcol[lp], bi, frank, s.tk.thr, pnc1, pnc2, valid_cnt, digest, key,
                                      ok)) {
            defer_rank(a, frank);
            have = false;
            if constexpr (TAIL) {
#pragma unroll
              for (int o = 0; o < MAXOBJ; ++o) ok[o] = false;
            }
          }
        }
      }
      if (!ABLATE(a, 4)) topk_step(s.tk, a.n_obj, a.K, key, ok, frank);
      if constexpr (PIN) {
        if (jobok && rank < a.re) pin_next<N>(a.ns, a.pz, q);
      } else {
        if (jobok && rank < a.re) colex_next<N>(a.ns, p);
      }
      ++rank;
    }
  }
  if (valid_cnt) atomicAdd(&a.out_counters[0], (unsigned long long)valid_cnt);
  if (digest) atomicAdd(&a.out_counters[1], (unsigned long long)digest);
  __syncthreads();
  Rec* dst = a.out_top + (size_t)blockIdx.x * a.n_obj * KP;
  for (uint32_t i = tid; i < (uint32_t)a.n_obj * KP; i += FAST_BD) dst[i] = s.tk.top[i];
}

// ------------------------------------------------------------- launcher ---
// the kernel for config size n (null: unsupported), for the occupancy query
// and the launch alike
static const void* fast_fn(uint32_t n, int tail, bool pin = false) {
  switch (n) {
#define FN_CASE(NN)                                                                  \
  case NN:                                                                           \
    if (pin) return tail == FAST_PLAIN ? (const void*)sweep_fast_kernel<NN, FAST_PLAIN, true> : nullptr; \
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

int fast_occupancy(uint32_t n, int tail, size_t shm) {
  const void* k = fast_fn(n, tail);
  return k ? kernel_occupancy(k, FAST_BD, shm, 1) : 0;
}

hipError_t launch_fast(const FastArgs& a, uint32_t n, int tail, uint32_t grid, size_t shm, hipStream_t st,
                       hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn(n, tail);
  return k ? launch_kernel(k, a, grid, FAST_BD, shm, st, e0, e1) : hipErrorInvalidValue;
}

// ---- the pinned variant: the same selector, so the occupancy query and the
// launch see the kernel that runs (its LDS is fast_smem_bytes' for FAST_PLAIN)
int fast_pinned_occupancy(uint32_t n, size_t shm) {
  const void* k = fast_fn(n, FAST_PLAIN, true);
  return k ? kernel_occupancy(k, FAST_BD, shm, 1) : 0;
}

hipError_t launch_fast_pinned(const PinFastArgs& a, uint32_t n, uint32_t grid, size_t shm, hipStream_t st,
                              hipEvent_t e0, hipEvent_t e1) {
  const void* k = fast_fn(n, FAST_PLAIN, true);
  return k ? launch_kernel(k, a, grid, FAST_BD, shm, st, e0, e1) : hipErrorInvalidValue;
}

}  // namespace bote
