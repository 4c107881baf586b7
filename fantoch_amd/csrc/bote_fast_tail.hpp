// bote_fast_tail.hpp — the tail variants of the fast sweep kernel
// (bote_sweep.hip, FAST_* in bote_kernels.hpp): what a sweep with MAX,
// percentile or MDTM objectives carries per config beside the moments.  One
// carrier type, Tail<N, TAIL>, with one hook per stage of the kernel, and its
// part in the client loop, TailLoop; the kernel itself names no variant.
#pragma once
#include <type_traits>

#include "bote_fast.hpp"

namespace bote {

constexpr uint32_t QSH = 10;  // log2(FAST_BD * 4): byte stride between qtab member planes
static_assert((1u << QSH) == FAST_BD * 4, "qtab plane stride");

// the variants' per-position columns in LDS, staged by Tail::column
struct TailCols {
  uint32_t* cmax;  // FAST_MAX: per position, the largest client latency of its column
  uint2* c4;       // FAST_LIST: per position, its column's four largest client latencies, descending (4 x u16)
  uint64_t* ch;    // FAST_MDTM: per position, H of its client column (mdtm_key; shift invariant, so also H of ff1 and ff2)
};

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

// ------------------------------------------------------ small helpers -----
// the latency of client c in the CQT column at byte offset `col`
__device__ __forceinline__ uint32_t client_lat(const unsigned char* B, uint32_t col, uint32_t c) {
  return ld16(B, col + (c >> 2) * 8 + (c & 3) * 2) >> LAT_SHIFT;
}
// the members' latencies to the leader (the values of colocated()'s N-step loop again)
template <int N>
__device__ __forceinline__ void leader_lats(const unsigned char* B, uint32_t lcol, const uint32_t (&rowq)[N],
                                            uint32_t (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = ld16(B, lcol + rowq[k]) >> LAT_SHIFT;
}
// member j's own quorum latencies, read back from the lane's qtab planes: word
// j holds tables 0 and 1, word N + j (`third`) table 2
template <int N>
__device__ __forceinline__ uint32_t own_q(const unsigned char* B, uint32_t qlane, int j, bool third) {
  return ld32(B, qlane + ((uint32_t)(third ? N + j : j) << QSH));
}
// H (mdtm_key) of n values x[0..n) with sum s1, a two-step computation in
// registers (the colocated slots: n <= 16 members)
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
// two clients' latencies = distance + quorum latency, a dead remainder client masked to 0
__device__ __forceinline__ us2 lat2(us2 d, uint32_t ql, uint32_t mask) { return as_us2(as_u32(d + as_us2(ql)) & mask); }

// ----------------------------------------------------- the tail carrier ---
// What a variant of the kernel (TAIL = FAST_*) carries beside the moments, with
// one hook per stage of the kernel.  FAST_PLAIN carries nothing and every hook
// of it is empty; `TAIL ==` is tested here, in fast_layout and in fast_fn only.
// (Only<C, T>: a member that exists, as a T, in the variants C names)
struct Nil {};
template <bool C, class T>
using Only = std::conditional_t<C, T, Nil>;

// The carrier's part in the client loop (client_quads).
// FAST_MAX: each table's largest client latency into MX, one packed max
// (v_pk_max_u16) per half quad into a running register per table, taken after
// the remainder mask (a dead client counts 0); no LDS traffic is added.
// FAST_LIST: each table's four largest client latencies into ML,
// descending, as 4 x u16 in two words.  The loop keeps, per table, a descending
// list of four packed registers: the low halves are one stream (clients 0 and
// 2 of every quad), the high halves another (clients 1 and 3), and a masked
// half quad is inserted into both at once by 7 packed compare-exchange steps
// (v_pk_max_u16 / v_pk_min_u16).  After the loop the two streams' lists are
// merged.  A dead client enters as 0 and cannot displace a live value among
// the largest `need <= nc`.  No LDS traffic is added here either.
// FAST_MDTM: H of the tables in the mask `mdm` (bit t: table t has an
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
template <int NL, int TAIL>
struct TailLoop {
  static constexpr bool two_pass = TAIL == FAST_MDTM;
  Only<TAIL == FAST_MAX, us2[NL]> pm;                    // running packed maxima
  Only<TAIL == FAST_LIST, us2[NL][PCTL_FAST_DEPTH]> pl;  // running packed lists, descending
  Only<TAIL == FAST_MAX, uint32_t[NL]> MX;
  Only<TAIL == FAST_LIST, uint32_t[NL][2]> ML;
  Only<TAIL == FAST_MDTM, uint64_t[NL]> MH;
  Only<TAIL == FAST_MDTM, uint32_t> mdm, nc;
  Only<TAIL == FAST_MDTM, MdtmThr[NL]> thr;
  Only<TAIL == FAST_MDTM, us2[NL]> pT;  // T in both halves (T <= 2 * 4095)
  Only<TAIL == FAST_MDTM, uint32_t[NL]> A, C;

  __device__ __forceinline__ void init() {
#pragma unroll
    for (int t = 0; t < NL; ++t) {
      if constexpr (TAIL == FAST_MAX) pm[t] = us2{0, 0};
      if constexpr (TAIL == FAST_LIST) {
#pragma unroll
        for (int i = 0; i < PCTL_FAST_DEPTH; ++i) pl[t][i] = us2{0, 0};
      }
    }
  }
  // a half quad of table t: clients 0, 1 in a01 and 2, 3 in a23
  __device__ __forceinline__ void acc(int t, us2 a01, us2 a23) {
    if constexpr (TAIL == FAST_MAX) pm[t] = __builtin_elementwise_max(__builtin_elementwise_max(pm[t], a01), a23);
    if constexpr (TAIL == FAST_LIST) {
      pk_insert(pl[t], a01);
      pk_insert(pl[t], a23);
    }
  }
  __device__ __forceinline__ void finish() {
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
  }
  // ---- the second pass (two_pass): false when no table needs one
  __device__ __forceinline__ bool begin2(const uint32_t (&S1)[NL]) {
    if constexpr (two_pass) {
#pragma unroll
      for (int t = 0; t < NL; ++t) MH[t] = 0;
      if (!mdm) return false;
#pragma unroll
      for (int t = 0; t < NL; ++t) {
        thr[t] = (mdm >> t) & 1u ? mdtm_thr(S1[t], nc) : MdtmThr{0, 0};  // (uniform: no division for the others)
        pT[t] = us2{(unsigned short)thr[t].T, (unsigned short)thr[t].T};
        A[t] = C[t] = 0;
      }
    }
    return two_pass;
  }
  __device__ __forceinline__ bool third_plane() const {  // (uniform) the third table has an MDTM objective
    if constexpr (two_pass) return (mdm >> 2) & 1u;
    return false;
  }
  __device__ __forceinline__ void above(int t, us2 dlo, us2 dhi, uint32_t ql01, uint32_t ql23, uint32_t mlo,
                                        uint32_t mhi) {
    if constexpr (two_pass) {
      if (!(mdm & (1u << t))) return;  // uniform
      const us2 ones = {1, 1};
      const us2 a01 = lat2(dlo, ql01, mlo), a23 = lat2(dhi, ql23, mhi);
      const us2 e01 = __builtin_elementwise_sub_sat(a01, pT[t]), e23 = __builtin_elementwise_sub_sat(a23, pT[t]);
      A[t] = __builtin_amdgcn_udot2(e01, ones, A[t], false);
      A[t] = __builtin_amdgcn_udot2(e23, ones, A[t], false);
      C[t] = __builtin_amdgcn_udot2(__builtin_elementwise_min(e01, ones), ones, C[t], false);
      C[t] = __builtin_amdgcn_udot2(__builtin_elementwise_min(e23, ones), ones, C[t], false);
    }
  }
  __device__ __forceinline__ void end2() {
    if constexpr (two_pass) {
#pragma unroll
      for (int t = 0; t < NL; ++t) MH[t] = mdtm_h(nc, thr[t], A[t], C[t]);
    }
  }
};

// The MAX and percentile keys of a config out of `top`, the slots' maxima
// (FAST_MAX) or packed lists (FAST_LIST: FPaxos less the quorum latency, lq2 /
// lq3).  `sl` is uniform: one scalar branch per slot, which only picks the
// slot's values; FAST_LIST's order statistic is taken once, after it.  A free
// function over the arrays themselves, and the arithmetic outside the slot
// loop: both were measured ("Reading the fast kernel").
template <int TAIL, class Top>
__device__ __forceinline__ void tail_keys(const FastArgs& a, const Top& top, const Mom (&mom)[NSLOT], uint32_t lq2,
                                          uint32_t lq3, uint64_t (&key)[MAXOBJ], bool (&ok)[MAXOBJ]) {
#pragma unroll
  for (int o = 0; o < MAXOBJ; ++o) {
    if (o >= a.n_obj) break;
    const uint32_t kind = a.obj_kind[o];
    if (TAIL == FAST_MAX ? kind != OBJ_MAX : kind < OBJ_MAX) continue;
    const uint32_t sl = a.obj_slot[o];
    const bool pctl = kind >= OBJ_PCTL;
    const uint32_t need = pctl ? kind & PCTL_NEED_MASK : 1u;  // (MAX: the first entry)
    const bool whole = pctl && (kind & PCTL_WHOLE);
    [[maybe_unused]] bool hit = false;  // FAST_LIST: the slot's list, quorum latency and sum
    [[maybe_unused]] uint32_t l[2] = {0, 0}, add = 0;
    [[maybe_unused]] uint64_t s1 = 0;
#pragma unroll
    for (int q = 0; q < NSLOT; ++q) {
      if ((uint32_t)q != sl) continue;
      if constexpr (TAIL == FAST_MAX) {
        ok[o] = true;
        key[o] = max_key(top[q], mom[q].s1);
      } else {
        hit = true;
        l[0] = top[q][0];
        l[1] = top[q][1];
        add = q % 5 == SLOT_FF1 ? lq2 : q % 5 == SLOT_FF2 ? lq3 : 0u;
        s1 = mom[q].s1;
      }
    }
    if constexpr (TAIL == FAST_LIST) {
      if (hit) {
        const uint32_t v = list_at(l, need) + add;
        const uint32_t twice = whole ? v + list_at(l, need - 1) + add : 2 * v;
        ok[o] = true;
        key[o] = pctl ? pctl_key(twice, s1) : max_key(v, s1);
      }
    }
  }
}

// where a hook puts keys: the launch's objectives, the config's moments, its keys
struct TailKeys {
  const FastArgs& a;
  const Mom (&mom)[NSLOT];
  uint64_t (&key)[MAXOBJ];
  bool (&ok)[MAXOBJ];
};
// The carrier of one config.
// FAST_MAX: the variant for sweeps with a MAX objective (base key set).  It
// carries each slot's maximum: the Input leaderless tables' from the client
// loop, Input FPaxos in closed form (the leader column's largest latency,
// staged per position beside cs1/cs2, plus the quorum latency), and the
// colocated slots' from the values the Q phase and the N-step loop already
// hold.  The MAX keys are built just before finish_config, which leaves them
// alone, and withdrawn when it defers the config: built after it, the ten
// maxima stay live across the score and digest arithmetic and N = 7 spills
// (8 B/lane of scratch; none this way).
// FAST_LIST: the variant for sweeps with a percentile objective that
// needs at most four of its slot's largest values (base key set).  It carries
// each slot's four largest values, descending, where FAST_MAX carries the
// largest: the Input leaderless tables' from the client loop's packed lists,
// Input FPaxos from the leader column's four largest latencies (staged per
// position, c4) plus the quorum latency, the colocated leaderless from the
// lane's quorum table read back after the client loop (nothing more is live
// across it), colocated FPaxos from the N-step loop.  Entry 0 is the maximum,
// so the MAX objectives of such a sweep are served from the lists.  Keys are
// built and withdrawn as for FAST_MAX.
// FAST_MDTM: the variant for sweeps with an MDTM objective and no MAX
// or percentile one (base key set).  Only the slots that have an MDTM
// objective are treated (a mask over the launch, from obj_kind / obj_slot):
// the Input leaderless tables by client_quads' second pass; Input FPaxos from
// H of the leader's client column (staged per position, ch: H is shift
// invariant, the quorum latency drops out); the colocated leaderless slots
// from the lane's quorum table read back, colocated FPaxos from the N-step
// loop's values again, both in registers (small_mdtm_h).  Each H goes into its
// objectives' keys at once, before finish_config, which leaves them alone;
// they are withdrawn when it defers the config.
template <int N, int TAIL>
struct Tail {
  using QC = QCfg<N>;
  static constexpr int NL = QC::NL;
  using Loop = TailLoop<NL, TAIL>;
  static constexpr bool plain = TAIL == FAST_PLAIN;  // carries nothing
  Only<TAIL == FAST_MAX, uint32_t[NSLOT]> mx;      // the slots' maxima
  Only<TAIL == FAST_MAX, uint32_t[NL]> cMX;        // the colocated leaderless maxima, from the Q phase
  Only<TAIL == FAST_LIST, uint32_t[NSLOT][2]> l4;  // the slots' four largest values, packed (FPaxos: less the quorum latency)
  // the slots (bit = slot) and the leaderless tables (bit = table) that have an MDTM objective
  Only<TAIL == FAST_MDTM, uint32_t> mds, mdm;

  // the launch's MDTM slot mask (uniform; 0 for the other variants)
  static __device__ __forceinline__ uint32_t slots(const FastArgs& a) {
    uint32_t m = 0;
    if constexpr (TAIL == FAST_MDTM) {
      for (int o = 0; o < a.n_obj; ++o)
        if (a.obj_kind[o] == OBJ_MDTM) m |= 1u << a.obj_slot[o];
    }
    return m;
  }
  // the table mask of the slots AF1, AF2, E at `base` (0: Input, 5: colocated)
  static __device__ __forceinline__ uint32_t tables(uint32_t m, int base) {
    return ((m >> (base + SLOT_AF1)) & 1u) << QC::idx_a1 | ((m >> (base + SLOT_AF2)) & 1u) << QC::idx_a2 |
           ((m >> (base + SLOT_E)) & 1u) << QC::idx_e;
  }
  __device__ __forceinline__ explicit Tail(uint32_t slot_mask) {
    if constexpr (TAIL == FAST_MAX) {
#pragma unroll
      for (int t = 0; t < NL; ++t) cMX[t] = 0;
    }
    if constexpr (TAIL == FAST_MDTM) {
      mds = slot_mask;
      mdm = tables(slot_mask, 0);
    }
  }
  __device__ __forceinline__ bool has(int q) const { return (mds >> q) & 1u; }
  // slot q's H into the keys of its MDTM objectives (`q` is a constant and the
  // objectives uniform: scalar branches)
  __device__ __forceinline__ void mdtm_keys(int q, uint64_t h, const TailKeys& k) const {
#pragma unroll
    for (int o = 0; o < MAXOBJ; ++o) {
      if (o >= k.a.n_obj) break;
      if (k.a.obj_kind[o] != OBJ_MDTM || k.a.obj_slot[o] != (uint32_t)q) continue;
      k.ok[o] = true;
      k.key[o] = mdtm_key(h, k.mom[q].s1);
    }
  }

  // ---- prologue: position i's client column (at `col`, sum c1) into the variant's column
  static __device__ __forceinline__ void column(const TailCols& s, const unsigned char* B, uint32_t col, uint32_t nc,
                                                uint32_t c1, uint32_t i) {
    if constexpr (TAIL == FAST_MAX) {
      uint32_t cm = 0;
      for (uint32_t c = 0; c < nc; ++c) cm = max(cm, client_lat(B, col, c));
      s.cmax[i] = cm;
    }
    if constexpr (TAIL == FAST_LIST) {
      uint32_t cl[PCTL_FAST_DEPTH] = {0, 0, 0, 0};
      for (uint32_t c = 0; c < nc; ++c) list_insert(cl, client_lat(B, col, c));
      s.c4[i] = make_uint2(cl[0] | (cl[1] << 16), cl[2] | (cl[3] << 16));
    }
    if constexpr (TAIL == FAST_MDTM) {
      const MdtmThr t = mdtm_thr(c1, nc);
      uint32_t A = 0, C = 0;
      for (uint32_t c = 0; c < nc; ++c) {
        const uint32_t v = client_lat(B, col, c);
        A += v > t.T ? v - t.T : 0u;
        C += v > t.T ? 1u : 0u;
      }
      s.ch[i] = mdtm_h(nc, t, A, C);
    }
  }
  // ---- Q phase: a member's quorum latency of table t
  __device__ __forceinline__ void q_value(int t, uint32_t ql) {
    if constexpr (TAIL == FAST_MAX) cMX[t] = max(cMX[t], ql);
  }
  // ---- Input leaderless: the client loop's part, and what it found
  __device__ __forceinline__ Loop loop(uint32_t nc) const {
    Loop L;
    if constexpr (TAIL == FAST_MDTM) {
      L.mdm = mdm;
      L.nc = nc;
    }
    return L;
  }
  __device__ __forceinline__ void leaderless(const Loop& L, const TailKeys& k) {
    if constexpr (TAIL == FAST_MAX) {
      mx[SLOT_AF1] = L.MX[QC::idx_a1];
      mx[SLOT_AF2] = L.MX[QC::idx_a2];
      mx[SLOT_E] = L.MX[QC::idx_e];
    }
    if constexpr (TAIL == FAST_LIST) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        l4[SLOT_AF1][h] = L.ML[QC::idx_a1][h];
        l4[SLOT_AF2][h] = L.ML[QC::idx_a2][h];
        l4[SLOT_E][h] = L.ML[QC::idx_e][h];
      }
    }
    if constexpr (TAIL == FAST_MDTM) {
      if (has(SLOT_AF1)) mdtm_keys(SLOT_AF1, L.MH[QC::idx_a1], k);
      if (has(SLOT_AF2)) mdtm_keys(SLOT_AF2, L.MH[QC::idx_a2], k);
      if (has(SLOT_E)) mdtm_keys(SLOT_E, L.MH[QC::idx_e], k);
    }
  }
  // ---- Input FPaxos: the leader's position lp and quorum latencies
  __device__ __forceinline__ void fpaxos(const TailCols& s, uint32_t lp, uint32_t lq2, uint32_t lq3,
                                         const TailKeys& k) {
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
      if (has(SLOT_FF1)) mdtm_keys(SLOT_FF1, s.ch[lp], k);
      if (has(SLOT_FF2)) mdtm_keys(SLOT_FF2, s.ch[lp], k);
    }
  }
  // ---- colocated FPaxos: the members' latencies to the leader; f1 is their sum plus N lq2
  __device__ __forceinline__ void colocated_fpaxos(const unsigned char* B, uint32_t lcol, const uint32_t (&rowq)[N],
                                                   uint32_t f1, uint32_t lq2, uint32_t lq3, const TailKeys& k) {
    if constexpr (TAIL == FAST_MAX) {
      uint32_t x[N], fm = 0;
      leader_lats<N>(B, lcol, rowq, x);
#pragma unroll
      for (int j = 0; j < N; ++j) fm = max(fm, x[j]);
      mx[5 + SLOT_FF1] = fm + lq2;
      mx[5 + SLOT_FF2] = fm + lq3;
    }
    if constexpr (TAIL == FAST_LIST) {
      uint32_t x[N], fl[PCTL_FAST_DEPTH] = {0, 0, 0, 0};
      leader_lats<N>(B, lcol, rowq, x);
#pragma unroll
      for (int j = 0; j < N; ++j) list_insert(fl, x[j]);
      l4[5 + SLOT_FF1][0] = l4[5 + SLOT_FF2][0] = fl[0] | (fl[1] << 16);
      l4[5 + SLOT_FF1][1] = l4[5 + SLOT_FF2][1] = fl[2] | (fl[3] << 16);
    }
    if constexpr (TAIL == FAST_MDTM) {
      if (has(5 + SLOT_FF1) || has(5 + SLOT_FF2)) {
        uint32_t x[N];
        leader_lats<N>(B, lcol, rowq, x);
        const uint64_t h = small_mdtm_h<N>(x, f1 - (uint32_t)N * lq2);  // (the quorum latency drops out of H)
        if (has(5 + SLOT_FF1)) mdtm_keys(5 + SLOT_FF1, h, k);
        if (has(5 + SLOT_FF2)) mdtm_keys(5 + SLOT_FF2, h, k);
      }
    }
  }
  // ---- colocated leaderless: the members' own quorum latencies (own_q; cS1: their sums per table)
  __device__ __forceinline__ void colocated_leaderless(const unsigned char* B, uint32_t qlane,
                                                       const uint32_t (&cS1)[NL], const TailKeys& k) {
    if constexpr (TAIL == FAST_MAX) {
      mx[5 + SLOT_AF1] = cMX[QC::idx_a1];
      mx[5 + SLOT_AF2] = cMX[QC::idx_a2];
      mx[5 + SLOT_E] = cMX[QC::idx_e];
    }
    if constexpr (TAIL == FAST_LIST) {
      us2 pa[PCTL_FAST_DEPTH], pb[PCTL_FAST_DEPTH];
#pragma unroll
      for (int i = 0; i < PCTL_FAST_DEPTH; ++i) pa[i] = pb[i] = us2{0, 0};
#pragma unroll
      for (int j = 0; j < N; ++j) {
        pk_insert(pa, as_us2(own_q<N>(B, qlane, j, false)));
        if (NL == 3) pk_insert(pb, as_us2(own_q<N>(B, qlane, j, true)));
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
#pragma unroll
      for (int t = 0; t < NL; ++t) {
        if (!((tables(mds, 5) >> t) & 1u)) continue;
        uint32_t x[N];
#pragma unroll
        for (int j = 0; j < N; ++j) {
          const uint32_t w = own_q<N>(B, qlane, j, t == 2);
          x[j] = t == 1 ? w >> 16 : w & 0xFFFFu;
        }
        const uint64_t h = small_mdtm_h<N>(x, cS1[t]);
        if (QC::idx_a1 == t && has(5 + SLOT_AF1)) mdtm_keys(5 + SLOT_AF1, h, k);
        if (QC::idx_a2 == t && has(5 + SLOT_AF2)) mdtm_keys(5 + SLOT_AF2, h, k);
        if (QC::idx_e == t && has(5 + SLOT_E)) mdtm_keys(5 + SLOT_E, h, k);
      }
    }
  }
  // ---- the MAX and percentile keys, just before finish_config (the maxima and
  // lists die here, before the score and digest arithmetic); FAST_MDTM's keys
  // are in place by now
  __device__ __forceinline__ void build_keys(uint32_t lq2, uint32_t lq3, const TailKeys& k) const {
    if constexpr (TAIL == FAST_MAX) tail_keys<TAIL>(k.a, mx, k.mom, lq2, lq3, k.key, k.ok);
    if constexpr (TAIL == FAST_LIST) tail_keys<TAIL>(k.a, l4, k.mom, lq2, lq3, k.key, k.ok);
  }
  // ---- a deferred config offers nothing: the keys set before finish_config are withdrawn
  static __device__ __forceinline__ void withdraw(bool (&ok)[MAXOBJ]) {
    if constexpr (TAIL != FAST_PLAIN) {
#pragma unroll
      for (int o = 0; o < MAXOBJ; ++o) ok[o] = false;
    }
  }
};

}  // namespace bote
