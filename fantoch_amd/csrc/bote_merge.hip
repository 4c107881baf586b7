// bote_merge.hip — the sweeps' top-K list machinery on the device: the 8-way
// merge tree (merge_kernel), the one-launch merge of a group-kernel sweep's
// bounded lists (merge_wide_kernel, with the block-wide radix select
// wide_select), the top-K seed (seed_kernel) and the small control kernels
// around a launch (control words, counters).  DESIGN.md §4 "The list dump and
// the one-launch merge"; tests/test_merge_model.py restates the procedures.
#include <atomic>
#include "bote_kernels.hpp"

namespace bote {

// ----------------------------------------------------- top-K list merge --
// (one thread per record of the G_MERGE_LISTS x KP inputs: each launch of
// the merge chain is latency-bound, 23 us per level at 256 threads)
constexpr int MERGE_BD = G_MERGE_LISTS * KP;
// lists: n_lists lists, list i of objective o at src[i * list_stride + o * KP]
// out:   one list per group of G_MERGE_LISTS lists, at dst[g * out_stride + o * KP]
// Every input list is sorted (block top-K lists, padded with rec_max), so each
// record's output slot is its rank in the union: its index in its own list
// plus, per other list, how many records precede it there (ties go to the
// lower list index).  One pass of binary searches in LDS, no sort; a block
// that finds an unsorted input falls back to the full bitonic sort.
__global__ void __launch_bounds__(1024) merge_kernel(const Rec* src, uint32_t n_lists, uint64_t list_stride, Rec* dst,
                                                     uint64_t out_stride, const Rec* alt, uint32_t alt_lists,
                                                     const unsigned long long* sel, uint64_t cap) {
  if (sel && *sel > cap) {  // device-side choice of the input (fast sweep overflow fallback)
    src = alt;
    n_lists = alt_lists;
  }
  __shared__ Rec buf[G_MERGE_LISTS * KP];
  __shared__ int unsorted;
  const uint32_t g = blockIdx.x, o = blockIdx.y;
  if (threadIdx.x == 0) unsorted = 0;
  for (uint32_t i = threadIdx.x; i < G_MERGE_LISTS * KP; i += blockDim.x) {
    uint32_t l = g * G_MERGE_LISTS + i / KP;
    buf[i] = l < n_lists ? src[l * list_stride + o * KP + i % KP] : rec_max();
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < G_MERGE_LISTS * KP; i += blockDim.x)
    if (i % KP && rec_lt(buf[i], buf[i - 1])) unsorted = 1;
  __syncthreads();
  Rec* out = dst + g * out_stride + o * KP;
  if (unsorted) {  // block-uniform
    block_bitonic(buf, G_MERGE_LISTS * KP);
    for (uint32_t i = threadIdx.x; i < KP; i += blockDim.x) out[i] = buf[i];
    return;
  }
  for (uint32_t i = threadIdx.x; i < G_MERGE_LISTS * KP; i += blockDim.x) {
    const uint32_t l = i / KP;
    const Rec x = buf[i];
    uint32_t pos = i % KP;
    for (uint32_t m = 0; m < (uint32_t)G_MERGE_LISTS && pos < (uint32_t)KP; ++m) {
      if (m == l) continue;
      pos += m < l ? upper_bound_rec(buf + m * KP, KP, x) : lower_bound_rec(buf + m * KP, KP, x);
    }
    if (pos < (uint32_t)KP) out[pos] = x;
  }
}

hipError_t launch_merge(const Rec* src, uint32_t n_lists, const Rec* alt, uint32_t alt_lists, uint64_t list_stride,
                        const unsigned long long* sel, uint64_t cap, Rec* dst, uint64_t out_stride, uint32_t n_obj,
                        hipStream_t st) {
  // groups cover the larger input; the surplus groups emit all-padding lists
  const uint32_t m = n_lists > alt_lists ? n_lists : alt_lists;
  uint32_t groups = (m + G_MERGE_LISTS - 1) / G_MERGE_LISTS;
  hipLaunchKernelGGL(merge_kernel, dim3(groups, n_obj), dim3(MERGE_BD), 0, st, src, n_lists, list_stride, dst, out_stride,
                     alt, alt_lists, sel, cap);
  return hipGetLastError();
}

// ------------------------------------------------- one-launch list merge --
// One workgroup per objective merges a sweep's per-block top-K lists (sorted,
// padded with rec_max) into the K least of their union.  The group kernel's
// dump (bote_group.hip, FastArgs::kbound) writes each list only up to the
// least K-th key of any block, which still leaves most of every list: the
// blocks take statistically similar chunks, so the least of 512 per-block
// K-th order statistics leaves ~70 of each block's 100 records below it
// (round 4: ~36 k records per objective, 1.07 ms per step).  So the merge
// first tightens the bound from the lists' heads:
//   t = a key with at least K head records at or below it,
// where the head records (the first WIDE_HEAD of each list) are distinct
// configs, so the union's K-th key is <= t.  With 512 lists and K = 100 the
// K-th least head lies at about the 20th percentile of the block minima, and
// the union holds ~K + K/8 records at or below it.  t is found by a radix
// select with 10-bit digits over (key - least head) that stops as soon as the
// chosen digit's bin holds at most WIDE_SLACK heads beyond the K-th (one or
// two passes for mean keys), and t is that bin's upper edge.  Each list's
// prefix at or below min(t, kbound) is counted, the counts are scanned, and
// when the gathered records fit one pass (<= WIDE_RANK_MAX) each record's
// output slot is its rank among them (a count over LDS; the (key, rank) order
// is total, so ranks are distinct); larger fills (the overflow fallback's full
// lists, heavy ties at t) take the windowed bitonic path: passes of <=
// WIDE_SORT - K records sorted with the running K least.  The result is the K
// least of the union whatever the fill (tests/test_merge_model.py restates the
// procedure and bounds the gathered count).
constexpr int WIDE_BD = 1024, WIDE_SORT = 4096, WIDE_LISTS_PER_THREAD = 4, WIDE_HEAD = 2;
constexpr int WIDE_BINS = 1024, WIDE_WAVES = WIDE_BD / 64, WIDE_SLACK = 32, WIDE_RANK_MAX = 1024;
// A record with key == ~0 (a NaN COV key) has a real rank < C(R, n) < 2^64 - 1,
// so only padding matches both fields.
__device__ __forceinline__ bool is_rec_max(const Rec& r) { return r.key == ~0ull && r.rank == ~0ull; }
static_assert(WIDE_MERGE_LISTS == (uint32_t)(WIDE_BD * WIDE_LISTS_PER_THREAD), "one thread per WIDE_LISTS_PER_THREAD lists");
static_assert(WIDE_BINS == WIDE_BD, "the digit histogram shares the scan array");
constexpr int WIDE_FEW = 64;  // a bin this small is finished by one wave (wide_select)
// LDS: the head records of every list (thread-minor; the windowed path's
// sort buffer reuses them), the one-pass gather, the scan / digit histogram,
// control words, per-wave reductions and a small bin's values: 149 KB
constexpr size_t WIDE_HEADS_BYTES = (size_t)WIDE_LISTS_PER_THREAD * WIDE_HEAD * WIDE_BD * 16;
static_assert(WIDE_HEADS_BYTES >= (size_t)WIDE_SORT * 16, "the windowed sort buffer fits the head records");
size_t merge_wide_smem() {
  return WIDE_HEADS_BYTES + (size_t)WIDE_RANK_MAX * 16 + (WIDE_BD + 8) * sizeof(uint32_t) +
         4 * WIDE_WAVES * sizeof(uint64_t) + 2 * WIDE_FEW * sizeof(uint64_t);
}

// inclusive prefix sum over the wavefront
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  const uint32_t lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(v, d);
    if (lane >= (uint32_t)d) v += y;
  }
  return v;
}

// Block-wide selection for merge_wide_kernel: among the values the threads
// visit (each(f) calls f(v) for each of this thread's values), a value x with
// at least `need` values <= x, by an MSB-first radix select with 10-bit digits
// over (v - least value) that stops as soon as the chosen digit's bin holds at
// most WIDE_SLACK values beyond the need-th, or at the exact value.  `left` is
// then the need-th value's position among the values of the final bin and
// `inbin` their number (exact: x is the need-th value itself).  none: fewer
// than `need` values.  Every thread of the block calls it (it has barriers).
struct WideSel {
  uint64_t x;
  uint32_t left, inbin;
  bool exact, none;
  bool has_aux;  // a small final bin was ranked by (value, aux): aux is the selected item's
  uint64_t aux;
};
template <class Each>
__device__ WideSel wide_select(Each each, uint64_t need, uint32_t* hist, uint32_t* ctl, uint64_t* red, bool slack) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint64_t* few = red + 4 * WIDE_WAVES;  // the values of a small final bin
  uint64_t* fewa = few + WIDE_FEW;       // and their aux words (ranks: the items are then distinct)
  uint64_t mn = ~0ull, mx = 0, nv = 0;
  each([&](uint64_t v, uint64_t) {
    mn = min(mn, v);
    mx = max(mx, v);
    ++nv;
  });
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, (uint64_t)__shfl_xor((long long)mn, d));
    mx = max(mx, (uint64_t)__shfl_xor((long long)mx, d));
    nv += (uint64_t)__shfl_xor((long long)nv, d);
  }
  if (lane == 0) {
    red[wv] = mn;
    red[WIDE_WAVES + wv] = mx;
    red[2 * WIDE_WAVES + wv] = nv;
  }
  __syncthreads();
  mn = ~0ull;
  mx = 0;
  nv = 0;
#pragma unroll
  for (int w = 0; w < WIDE_WAVES; ++w) {
    mn = min(mn, red[w]);
    mx = max(mx, red[WIDE_WAVES + w]);
    nv += red[2 * WIDE_WAVES + w];
  }
  WideSel r{~0ull, 0, 0, false, true, false, 0};
  if (nv >= need && need > 0) {  // (block-uniform)
    r.none = false;
    if (mx == mn) {
      r = WideSel{mn, (uint32_t)need, (uint32_t)nv, true, false, false, 0};
    } else {
      uint32_t s_hi = 64 - (uint32_t)__clzll(mx - mn);  // every (v - mn) < 2^s_hi
      uint64_t prefix = 0;
      for (;;) {
        const uint32_t s_lo = s_hi > 10 ? s_hi - 10 : 0, w = s_hi - s_lo;
        hist[tid] = 0;
        __syncthreads();
        // (shared-count audit, round 6: the adds follow the zeroing barrier;
        // wave 0 reads the bins only after the barrier below; every thread
        // reads the pick (ctl[2..4]) after the next one, and the histogram is
        // zeroed again only after the loop's closing barrier, so no thread can
        // add into a pass while another still reads the last)
        each([&](uint64_t v, uint64_t) {
          v -= mn;
          if (s_hi >= 64 || (v >> s_hi) == prefix) atomicAdd(&hist[(uint32_t)(v >> s_lo) & ((1u << w) - 1)], 1u);
        });
        __syncthreads();
        if (wv == 0) {  // one wave: the bin holding the need-th value, 16 bins per lane
          uint32_t cb[WIDE_BINS / 64], sl = 0;
#pragma unroll
          for (int q = 0; q < WIDE_BINS / 64; ++q) {
            cb[q] = hist[lane * (WIDE_BINS / 64) + q];
            sl += cb[q];
          }
          uint32_t before = wave_incl_scan(sl) - sl;
#pragma unroll
          for (int q = 0; q < WIDE_BINS / 64; ++q) {
            if (before < need && need <= before + cb[q]) {  // exactly one lane, one bin
              ctl[2] = lane * (WIDE_BINS / 64) + q;
              ctl[3] = (uint32_t)(need - before);
              ctl[4] = cb[q];
            }
            before += cb[q];
          }
          if (lane == 0) ctl[5] = 0;  // (slots of a small bin's values)
        }
        __syncthreads();
        const uint32_t d = ctl[2], left = ctl[3], inbin = ctl[4];
        prefix = (prefix << w) | d;
        need = left;
        s_hi = s_lo;
        if (s_hi == 0 || (slack && inbin - left <= (uint32_t)WIDE_SLACK)) {  // (block-uniform)
          r.left = left;
          r.inbin = inbin;
          r.exact = s_hi == 0;
          break;
        }
        if (inbin <= (uint32_t)WIDE_FEW) {  // (block-uniform) the bin's values to one wave: exact
          each([&](uint64_t v, uint64_t aux) {
            v -= mn;
            if ((v >> s_hi) == prefix) {
              // (audit: ctl[5] was zeroed by wave 0 before the pick barrier;
              // the adds precede the barrier below, after which only wave 0
              // reads the slots, and every path out of here passes a barrier
              // before ctl is written again)
              const uint32_t k = atomicAdd(&ctl[5], 1u);
              few[k] = v;
              fewa[k] = aux;
            }
          });
          __syncthreads();
          if (wv == 0) {
            // the left-th least item in (value, aux) order: fewer than `left`
            // items below it and at least `left` at or below it (equal items:
            // every lane holding one agrees); with distinct aux words (ranks)
            // it is one item, so the caller has its aux without a second select
            const uint64_t x = lane < inbin ? few[lane] : ~0ull, xa = lane < inbin ? fewa[lane] : ~0ull;
            uint32_t lt = 0, le = 0, vlt = 0, vle = 0;
            for (uint32_t j = 0; j < inbin; j += 4) {  // (4 reads in flight; inbin <= 64 = the buffer)
#pragma unroll
              for (uint32_t u = 0; u < 4; ++u) {
                const uint64_t y = few[j + u], ya = fewa[j + u];
                const bool in = j + u < inbin;
                lt += (uint32_t)(in && (y < x || (y == x && ya < xa)));
                le += (uint32_t)(in && (y < x || (y == x && ya <= xa)));
                vlt += (uint32_t)(in && y < x);
                vle += (uint32_t)(in && y <= x);
              }
            }
            if (lane < inbin && lt < left && left <= le) {
              red[0] = x;
              red[1] = xa;
              ctl[3] = left - vlt;  // (its position among the values equal to it)
              ctl[4] = vle - vlt;
            }
          }
          __syncthreads();
          r.x = mn + red[0];
          r.aux = red[1];
          r.has_aux = true;
          r.left = ctl[3];
          r.inbin = ctl[4];
          r.exact = true;
          __syncthreads();
          return r;
        }
        __syncthreads();  // (the histogram and ctl are rewritten by the next pass)
      }
      const uint64_t x = (prefix << s_hi) | ((1ull << s_hi) - 1);  // (s_hi < 64 after a pass)
      r.x = x > ~0ull - mn ? ~0ull : mn + x;
    }
  }
  __syncthreads();  // (red, hist and ctl are reused by the caller)
  return r;
}

__global__ void __launch_bounds__(WIDE_BD) merge_wide_kernel(const Rec* src, uint32_t n_lists, uint64_t list_stride,
                                                             Rec* dst, const Rec* alt, uint32_t alt_lists,
                                                             const unsigned long long* sel, uint64_t cap,
                                                             const unsigned long long* kbound, uint32_t K,
                                                             const unsigned long long* csrc,
                                                             const unsigned long long* calt, uint64_t* cdst) {
#ifdef BOTE_MERGE_PRINTF
  const uint64_t T0 = wall_clock64();
  uint64_t TT[4] = {0, 0, 0, 0};
  int tn = 0;
#define WIDE_T(name) TT[tn++ & 3] = wall_clock64() - T0;
#else
#define WIDE_T(name)
#endif
  const bool use_alt = sel && *sel > cap;
  if (use_alt) {  // device-side choice of the input (fast sweep overflow fallback)
    src = alt;
    n_lists = alt_lists;
  }
  // the result's counters (valid, digest) from the same choice (what
  // pick_counters_kernel does for the merge tree; one launch fewer)
  if (cdst && blockIdx.x == 0 && threadIdx.x < 2) cdst[threadIdx.x] = (use_alt ? calt : csrc)[threadIdx.x];
  extern __shared__ __align__(16) unsigned char wsm[];
  Rec* hr = (Rec*)wsm;                              // head records (then the windowed path's buffer)
  Rec* buf = hr;                                    // the windowed path's sort buffer
  Rec* gbuf = (Rec*)(wsm + WIDE_HEADS_BYTES);       // the one-pass gather
  uint32_t* scan = (uint32_t*)(wsm + WIDE_HEADS_BYTES + (size_t)WIDE_RANK_MAX * 16);  // also the digit histogram
  uint32_t* ctl = scan + WIDE_BD;  // [0] next window start, [1] records this pass; [2..4] the digit pick
  uint64_t* red = (uint64_t*)(ctl + 8);  // per wave: least and greatest value, count
  const uint32_t o = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t KK = K < (uint32_t)KP ? K : (uint32_t)KP;
  Rec* out = dst + o * KP;
  if (KK == 0) {
    for (uint32_t i = tid; i < (uint32_t)KP; i += WIDE_BD) out[i] = rec_max();
    return;
  }
  constexpr int LT = WIDE_LISTS_PER_THREAD, H = WIDE_HEAD;
  auto list = [&](int j) { return src + (size_t)(tid * LT + j) * list_stride + o * KP; };
  auto live = [&](int j) { return tid * LT + (uint32_t)j < n_lists; };
  // records above the bound on the K-th key (the least K-th key of the
  // group blocks' full lists) cannot be among the K least of the union
  const uint64_t b0 = kbound && !use_alt ? kbound[o] : ~0ull;
  // the first WIDE_HEAD records of all of a thread's lists load together
  // (one round trip to memory: the lists were written by blocks on every
  // XCD) into LDS, thread-minor (in registers they spilled at 1,024
  // threads); everything up to the gather then reads LDS
  auto hrec = [&](int j, int c) -> Rec& { return hr[(c * LT + j) * WIDE_BD + tid]; };
  auto hk = [&](int j, int c) -> uint64_t { return hrec(j, c).key; };
  {
    Rec t[LT][H];
#pragma unroll
    for (int j = 0; j < LT; ++j)
#pragma unroll
      for (int c = 0; c < H; ++c) t[j][c] = live(j) && (uint32_t)c < KK ? list(j)[c] : Rec{~0ull, ~0ull};
#pragma unroll
    for (int j = 0; j < LT; ++j)
#pragma unroll
      for (int c = 0; c < H; ++c) hrec(j, c) = t[j][c];
  }
  WIDE_T("heads")
  // the bound record (bk, br): the union's K least are at or below it
  uint64_t bk = ~0ull, br = ~0ull;
  {
    // the heads' kept prefix per list (a list's records end at its
    // terminator: what follows it in memory is stale; a key of all ones, a
    // NaN COV, also ends it here: fewer heads only loosen the bound)
    uint32_t hn[LT];
#pragma unroll
    for (int j = 0; j < LT; ++j) {
      uint32_t c = 0;
#pragma unroll
      for (int i = 0; i < H; ++i) c += (uint32_t)(c == (uint32_t)i && hk(j, i) != ~0ull && hk(j, i) <= b0);
      hn[j] = c;
    }
    auto each_head = [&](auto f) {
#pragma unroll
      for (int j = 0; j < LT; ++j)
#pragma unroll
        for (int c = 0; c < H; ++c)
          if ((uint32_t)c < hn[j]) f(hk(j, c), hrec(j, c).rank);
    };
    // (to the exact key: a bin's worth of heads above the K-th could stand
    // for many more tied records beyond the heads)
    const WideSel ks = wide_select(each_head, KK, scan, ctl, red, false);
    WIDE_T("keysel")
    if (!ks.none) {
      bk = ks.x;
      if (ks.has_aux && ks.inbin > 1) {
        br = ks.aux;  // (a small final bin ranked by (key, rank): the K-th head record itself)
      } else if (ks.inbin > 1) {
        // heads tie at the K-th key (FPaxos means: round 5 measured 1,186
        // records at one key on a 1/8 shard): the left-th least rank among
        // them makes (bk, br) the K-th least head record itself
        auto each_tie = [&](auto f) {
#pragma unroll
          for (int j = 0; j < LT; ++j)
#pragma unroll
            for (int c = 0; c < H; ++c)
              if ((uint32_t)c < hn[j] && hk(j, c) == bk) f(hrec(j, c).rank, 0ull);
        };
        const WideSel rs = wide_select(each_tie, ks.left, scan, ctl, red, true);
        if (!rs.none) br = rs.x;
      }
    }
  }
  const uint64_t kb = min(b0, bk);
  // a record is gathered when it is a real record at or below both bounds
  auto keep = [&](const Rec& r) {
    return !is_rec_max(r) && r.key <= kb && (r.key < bk || r.rank <= br);
  };
  // per list: the filled prefix length at or below the bound (keys from the
  // registers; a rank is read only where it decides)
  uint32_t cnt[LT], off[LT], mine = 0;
#pragma unroll
  for (int j = 0; j < LT; ++j) {
    uint32_t c = 0;
    bool go = live(j);
#pragma unroll
    for (int i = 0; i < H; ++i) {
      if (go && (uint32_t)i < KK) {
        const uint64_t k = hk(j, i);
        bool in = k <= kb;
        if (in && (k == ~0ull || (k == bk && br != ~0ull))) in = keep(hrec(j, i));
        c += in ? 1u : 0u;
        go = in;
      } else {
        go = false;
      }
    }
    if (go) {  // a long list (rare): walk the rest
      const Rec* L = list(j);
      while (c < KK && keep(L[c])) ++c;
    }
    cnt[j] = c;
    off[j] = mine;
    mine += c;
  }
  // exclusive scan of the threads' totals (list order = thread order): per
  // wave by shuffles, then the waves' totals
  const uint32_t incl = wave_incl_scan(mine);
  if (lane == 63) scan[wv] = incl;
  __syncthreads();
  uint32_t base = incl - mine, total = 0;
#pragma unroll
  for (uint32_t w = 0; w < (uint32_t)WIDE_WAVES; ++w) {
    const uint32_t x = scan[w];
    base += w < wv ? x : 0u;
    total += x;
  }
#pragma unroll
  for (int j = 0; j < LT; ++j) off[j] += base;
  WIDE_T("scan")
  if (total <= (uint32_t)WIDE_RANK_MAX) {  // (block-uniform) one pass: slot = rank among the gathered
#pragma unroll
    for (int j = 0; j < LT; ++j) {
#pragma unroll
      for (int c = 0; c < H; ++c)
        if ((uint32_t)c < cnt[j]) gbuf[off[j] + c] = hrec(j, c);
      if (cnt[j] > (uint32_t)H) {  // (rare: beyond the heads)
        const Rec* L = list(j);
        for (uint32_t c = H; c < cnt[j]; ++c) gbuf[off[j] + c] = L[c];
      }
    }
    // (padded with rec_max to a multiple of 8: the count loop below keeps 8
    // independent LDS reads in flight; padding is never below a record)
    const uint32_t tot8 = (total + 7) & ~7u;
    if (tid >= total && tid < tot8) gbuf[tid] = rec_max();
    __syncthreads();
    for (uint32_t i = tid; i < total; i += WIDE_BD) {
      const Rec x = gbuf[i];
      uint32_t r = 0;
      for (uint32_t m = 0; m < tot8; m += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r += (uint32_t)rec_lt(gbuf[m + u], x);
      }
      if (r < KK) out[r] = x;
    }
    for (uint32_t i = min(total, KK) + tid; i < (uint32_t)KP; i += WIDE_BD) out[i] = rec_max();
    WIDE_T("done")
#ifdef BOTE_MERGE_PRINTF
    if (tid == 0)
      printf("merge o=%u lists=%u total=%u bk=%llx br=%llx ticks heads %llu keysel %llu scan %llu done %llu\n", o,
             n_lists, total, (unsigned long long)bk, (unsigned long long)br, (unsigned long long)TT[0],
             (unsigned long long)TT[1], (unsigned long long)TT[2], (unsigned long long)TT[3]);
#endif
    return;
  }
  // running K least: buf[0 .. have) (buf overwrites the head records: the
  // windowed passes gather from memory)
  uint32_t have = 0;
  const uint32_t room = WIDE_SORT - KK;  // records gathered per pass
  uint32_t w0 = 0;  // window start (in the concatenated order)
  while (w0 < total) {
    __syncthreads();
    if (tid == 0) {
      ctl[0] = total;  // the next window starts at the first list that does not fit
      ctl[1] = 0;
    }
    __syncthreads();
    // lists inside [w0, w0 + room) are copied after the running list
#pragma unroll
    for (int j = 0; j < LT; ++j) {
      if (cnt[j] == 0 || off[j] < w0) continue;
      if (off[j] + cnt[j] - w0 <= room) {
        Rec* d = buf + KK + off[j] - w0;
        const Rec* L = list(j);
        for (uint32_t c = 0; c < cnt[j]; ++c) d[c] = L[c];
        atomicMax(&ctl[1], off[j] + cnt[j] - w0);
      } else {
        // (audit: thread 0 resets ctl[0..1] between the two barriers at the
        // window's start; the atomics follow them, every thread reads
        // got / next after the barrier below, and the next window's reset
        // waits for the barrier that opens it)
        atomicMin(&ctl[0], off[j]);
      }
    }
    __syncthreads();
    const uint32_t got = ctl[1], next = ctl[0];
    // compact: running records at [0, have), the pass's at [KK, KK + got)
    uint32_t n = KK + got, P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = tid; i < P; i += WIDE_BD)
      if ((i >= have && i < KK) || i >= n) buf[i] = rec_max();
    __syncthreads();
    block_bitonic(buf, (int)P);
    have = min(KK, n);
    w0 = next;
  }
  __syncthreads();
  for (uint32_t i = tid; i < (uint32_t)KP; i += WIDE_BD) out[i] = i < have && i < KK ? buf[i] : rec_max();
}
#undef WIDE_T

hipError_t launch_merge_wide(const Rec* src, uint32_t n_lists, const Rec* alt, uint32_t alt_lists, uint64_t list_stride,
                             const unsigned long long* sel, uint64_t cap, const unsigned long long* kbound, Rec* dst,
                             uint32_t n_obj, uint32_t K, const unsigned long long* csrc, const unsigned long long* calt,
                             uint64_t* cdst, hipStream_t st) {
  if (n_lists > (uint32_t)(WIDE_BD * WIDE_LISTS_PER_THREAD) || alt_lists > (uint32_t)(WIDE_BD * WIDE_LISTS_PER_THREAD))
    return hipErrorInvalidValue;
  const size_t shm = merge_wide_smem();
  // (the LDS limit above 64 KB, once per device)
  static std::atomic<uint64_t> done{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (!(done.load(std::memory_order_relaxed) & bit)) {
    e = hipFuncSetAttribute((const void*)merge_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
    if (e != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_relaxed);
  }
  hipLaunchKernelGGL(merge_wide_kernel, dim3(n_obj), dim3(WIDE_BD), shm, st, src, n_lists, list_stride, dst, alt,
                     alt_lists, sel, cap, kbound, K, csrc, calt, cdst);
  return hipGetLastError();
}

__global__ void pick_counters_kernel(const unsigned long long* src, const unsigned long long* alt,
                                     const unsigned long long* sel, uint64_t cap, uint64_t* dst) {
  if (threadIdx.x < 2) dst[threadIdx.x] = (*sel > cap ? alt : src)[threadIdx.x];
}

// the per-launch control words of a fast-path sweep zeroed in one launch
// (valid/digest counters, the deferred-queue count, the work-ticket counter,
// the overflow fallback's counters) instead of four memsets
__global__ void zero_ctl_kernel(unsigned long long* counters, unsigned long long* qcount, unsigned int* wctr,
                                unsigned long long* counters_alt, unsigned long long* kbound) {
  const uint32_t t = threadIdx.x;
  if (t < 2) counters[t] = 0;
  if (t == 2) *qcount = 0;
  if (t >= 4 && t < 6) counters_alt[t - 4] = 0;
  if (t >= 8 && t < 24 && wctr) wctr[32 * (t - 8)] = 0;  // the 8 ticket-counter shards, main and sample launch
  if (t >= 32 && t < 32 + MAXOBJ && kbound) kbound[t - 32] = ~0ull;  // the lists' K-th key bound (no bound)
}

hipError_t launch_zero_ctl(unsigned long long* counters, unsigned long long* qcount, unsigned int* wctr,
                           unsigned long long* counters_alt, unsigned long long* kbound, hipStream_t st) {
  hipLaunchKernelGGL(zero_ctl_kernel, dim3(1), dim3(64), 0, st, counters, qcount, wctr, counters_alt, kbound);
  return hipGetLastError();
}

// The top-K seed: per objective (one block each) the K-th least of the
// sample launch's per-chunk minima, by an exact MSB-first radix select (8-bit
// digits: a 256-bin LDS histogram of the keys that share the prefix so far,
// then the digit holding the K-th); all-ones (no bound) when fewer than K
// samples have the objective.  The bytes above the highest one in which the
// keys differ (found first from their AND and OR) are taken as known: mean
// keys (S1 < 2^21) skip 5 of the 8 passes, whose histograms would all hit one
// bin.  (A bitonic sort of 4096 keys took 56 us: 78 barrier-separated stages.)
__global__ void __launch_bounds__(1024) seed_kernel(const uint64_t* smin, uint32_t nsamp, uint32_t K, uint64_t* tseed) {
  __shared__ uint32_t hist[256];
  __shared__ uint64_t sel[3];  // prefix, remaining rank, keys in the chosen bin
  __shared__ uint64_t red[2][16];
  __shared__ uint64_t few[64];  // a small final bin's keys
  __shared__ uint32_t nfew;
  const uint32_t o = blockIdx.x, tid = threadIdx.x, BD = blockDim.x;
  if (nsamp < K || K == 0) {
    if (tid == 0) tseed[o] = ~0ull;
    return;
  }
  const uint64_t* x = smin + (size_t)o * nsamp;
  // up to RP keys per thread stay in registers across the passes (32,768 keys
  // re-read from memory every pass took 72 us); larger samples re-read
  constexpr int RP = 32;
  const bool inreg = nsamp <= (uint32_t)RP * BD;
  uint64_t xr[RP];
#pragma unroll
  for (int i = 0; i < RP; ++i) {
    const uint32_t k = tid + (uint32_t)i * BD;
    xr[i] = inreg && k < nsamp ? x[k] : ~0ull;
  }
  // the AND and OR of all keys: the bits above their highest difference are common
  uint64_t va = ~0ull, vo = 0;
  if (inreg) {
#pragma unroll
    for (int i = 0; i < RP; ++i)
      if (tid + (uint32_t)i * BD < nsamp) {
        va &= xr[i];
        vo |= xr[i];
      }
  } else {
    for (uint32_t k = tid; k < nsamp; k += BD) {
      va &= x[k];
      vo |= x[k];
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    va &= (uint64_t)__shfl_xor((long long)va, d);
    vo |= (uint64_t)__shfl_xor((long long)vo, d);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = va;
    red[1][tid >> 6] = vo;
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t a = ~0ull, b = 0;
    for (uint32_t w = 0; w < (BD >> 6); ++w) {
      a &= red[0][w];
      b |= red[1][w];
    }
    const uint64_t diff = a ^ b;  // bits in which some keys differ
    const int top = diff ? 63 - __clzll(diff) : -1;  // highest such bit
    const int pass0 = top < 0 ? -1 : top / 8;        // first byte to select on
    // the known high bytes; the rank within them is K
    sel[0] = pass0 < 0 ? a : (pass0 == 7 ? 0 : a >> (8 * (pass0 + 1)));
    sel[1] = K;
    red[0][0] = (uint64_t)(int64_t)pass0;
  }
  __syncthreads();
  const int pass0 = (int)(int64_t)red[0][0];
  for (int pass = pass0; pass >= 0; --pass) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const uint64_t prefix = sel[0];
    const int sh = 8 * pass;
    // (audit: the bins are zeroed before the barrier above; wave 0 reads
    // them after the barrier below and publishes sel[] before the next one;
    // every thread reads sel[] after it, and the next pass zeroes the bins
    // only after that barrier, so no add lands in a pass still being read)
    auto count = [&](uint64_t v) {
      if (pass == 7 || (v >> (sh + 8)) == prefix) atomicAdd(&hist[(v >> sh) & 0xFFu], 1u);
    };
    if (inreg) {
#pragma unroll
      for (int i = 0; i < RP; ++i)
        if (tid + (uint32_t)i * BD < nsamp) count(xr[i]);
    } else {
      for (uint32_t k = tid; k < nsamp; k += BD) count(x[k]);
    }
    __syncthreads();
    if (tid < 64) {  // one wave: inclusive scan of the 256 bins, 4 per lane
      uint32_t c[4], s = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) c[b] = hist[4 * tid + b];
#pragma unroll
      for (int b = 0; b < 4; ++b) s += c[b];
      uint32_t incl = s;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d);
        if ((int)tid >= d) incl += y;
      }
      const uint64_t need = sel[1];
      uint32_t before = incl - s;  // keys in the bins of the lanes below
      int digit = -1;
      uint64_t left = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if (digit < 0 && before < need && need <= before + c[b]) {
          digit = 4 * (int)tid + b;
          left = need - before;
        }
        before += c[b];
      }
      if (digit >= 0) {  // exactly one lane holds the K-th key's digit
        sel[0] = (sel[0] << 8) | (uint64_t)digit;
        sel[1] = left;
        sel[2] = hist[digit];
      }
      if (tid == 0) nfew = 0;
    }
    __syncthreads();
    if (pass > 0 && sel[2] <= 64) {  // (block-uniform) a small bin: one wave ranks its keys
      const uint64_t pfx = sel[0];
      const int shb = 8 * pass;
      // (audit: nfew is zeroed by thread 0 before the pick barrier; the
      // adds follow it and wave 0 reads nfew after the barrier below, then
      // the block returns: nfew is never added to again in this launch)
      auto push = [&](uint64_t v) {
        if ((v >> shb) == pfx) few[atomicAdd(&nfew, 1u)] = v;
      };
      if (inreg) {
#pragma unroll
        for (int i = 0; i < RP; ++i)
          if (tid + (uint32_t)i * BD < nsamp) push(xr[i]);
      } else {
        for (uint32_t k = tid; k < nsamp; k += BD) push(x[k]);
      }
      __syncthreads();
      if (tid < 64) {  // the sel[1]-th least of the bin's keys
        const uint32_t nb = nfew, need = (uint32_t)sel[1];
        const uint64_t v = tid < nb ? few[tid] : ~0ull;
        uint32_t lt = 0, le = 0;
        for (uint32_t j = 0; j < nb; j += 4) {  // (4 reads in flight; nb <= 64 = the buffer)
#pragma unroll
          for (uint32_t u = 0; u < 4; ++u) {
            const uint64_t y = few[j + u];
            lt += (uint32_t)(j + u < nb && y < v);
            le += (uint32_t)(j + u < nb && y <= v);
          }
        }
        if (tid < nb && lt < need && need <= le) tseed[o] = v;  // (every lane holding it writes the same)
      }
      return;
    }
  }
  if (tid == 0) tseed[o] = sel[0];
}

hipError_t launch_seed(const uint64_t* smin, uint32_t nsamp, uint32_t n_obj, uint32_t K, uint64_t* tseed,
                       hipStream_t st) {
  hipLaunchKernelGGL(seed_kernel, dim3(n_obj), dim3(1024), 0, st, smin, nsamp, K, tseed);
  return hipGetLastError();
}

hipError_t launch_pick_counters(const unsigned long long* src, const unsigned long long* alt,
                                const unsigned long long* sel, uint64_t cap, uint64_t* dst, hipStream_t st) {
  hipLaunchKernelGGL(pick_counters_kernel, dim3(1), dim3(64), 0, st, src, alt, sel, cap, dst);
  return hipGetLastError();
}

__global__ void sum_counters_kernel(const uint64_t* src, uint32_t n, uint64_t stride, uint64_t off, uint64_t* dst) {
  if (threadIdx.x < 2) {
    uint64_t s = 0;
    for (uint32_t i = 0; i < n; ++i) s += src[i * stride + off + threadIdx.x];
    dst[threadIdx.x] = s;
  }
}

hipError_t launch_sum_counters(const uint64_t* src, uint32_t n, uint64_t stride, uint64_t off, uint64_t* dst,
                               hipStream_t st) {
  hipLaunchKernelGGL(sum_counters_kernel, dim3(1), dim3(64), 0, st, src, n, stride, off, dst);
  return hipGetLastError();
}

}  // namespace bote
