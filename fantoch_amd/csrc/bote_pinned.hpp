// bote_pinned.hpp — pinned sweeps (DESIGN.md §4 "Pinned sweeps"): the search
// over the supersets of m pinned positions, 1 <= m < N.  The rank space is the
// colex ranks of the F = N - m subsets of indices into free[] (the unpinned
// positions, ascending): the pinned rank.  Records, the digest and the
// deferred queue carry the config's full colex rank; for two supersets of one
// pinned set the two orders agree (bote_host.hpp), so the lists merge with the
// unchanged merge kernels and the deferred configs go through the unchanged
// rank-list fix-up of eval_kernel.
//
// The member stage shared by the two kernels that walk pinned ranks: its state is
// the free indices q[] and the merged ascending members p[N].  F and m are
// runtime values, uniform over the launch: every array stays in registers with
// fully unrolled loops under uniform predicates (scalar branches), never a
// dynamically indexed private array.  Free index number i lives in q[m + i],
// so member slot j holds pin[j] below m and a free member from m on, with
// compile-time indices throughout.
#pragma once
#include "bote_kernels.hpp"

namespace bote {

// The fast kernel's arguments with the pinned fields (PinArgs,
// bote_kernels.hpp) at the end, as its launcher builds them: the kernarg
// offsets of FastArgs stay.
struct PinFastArgs : FastArgs {
  PinArgs pz;
};
// The generic kernel's, the same way.
struct PinEvalArgs : EvalArgs {
  PinArgs pz;
};
// A batch of pinned sets (BatchArgs, bote_kernels.hpp): the fast kernel's
// batch variant reads a unit's set from the device table bz.sets.
struct BatchFastArgs : FastArgs {
  BatchArgs bz;
};

// pinned rank -> q (binom: the (ns + 1) x (N + 1) table, which holds every
// C(x, k) with x <= ns - m, k <= F at the same stride)
template <int N>
__device__ __forceinline__ void pin_unrank(const uint64_t* binom, uint32_t ns, const PinArgs& z, uint64_t prank,
                                           uint32_t (&q)[N]) {
  const uint32_t m = z.pin_n;
  uint64_t r = prank;
  uint32_t hi = ns - m;
  q[0] = 0;  // (m >= 1: slot 0 is pinned)
#pragma unroll
  for (int j = N - 1; j >= 1; --j) {
    q[j] = 0;
    if ((uint32_t)j >= m) {
      const uint32_t k = (uint32_t)j - m + 1;
      uint32_t lo = k - 1, up = hi;  // answer in [lo, up)
      while (up - lo > 1) {
        const uint32_t mid = (lo + up) >> 1;
        if (binom[mid * (N + 1) + k] <= r) lo = mid; else up = mid;
      }
      q[j] = lo;
      r -= binom[lo * (N + 1) + k];
      hi = lo;
    }
  }
}

// the colex successor of q over the ns - m free indices
template <int N>
__device__ __forceinline__ void pin_next(uint32_t ns, const PinArgs& z, uint32_t (&q)[N]) {
  const uint32_t m = z.pin_n, nf = ns - m;
  uint32_t js = N;  // first free slot j with q[j] + 1 < q[j + 1]
#pragma unroll
  for (int j = N - 1; j >= 1; --j) {
    if ((uint32_t)j >= m) {
      const uint32_t nxt = (j == N - 1) ? nf : q[j + 1 < N ? j + 1 : j];
      if (q[j] + 1 < nxt) js = j;
    }
  }
#pragma unroll
  for (int j = 1; j < N; ++j)
    if ((uint32_t)j >= m) q[j] = (uint32_t)j < js ? (uint32_t)j - m : ((uint32_t)j == js ? q[j] + 1 : q[j]);
}

// q -> the config's members p[N], ascending, and its full colex rank.  A free
// index x is position free[x]: x plus the pinned positions at or below it,
// counted in ascending order (m uniform compares).  The pinned and the free
// positions, each ascending, are merged by a sorting network.
template <int N>
__device__ __forceinline__ void pin_members(const uint64_t* binom, const PinArgs& z, const uint32_t (&q)[N],
                                            uint32_t (&p)[N], uint64_t& full_rank) {
  constexpr int P = Pow2<N>::v;
  const uint32_t m = z.pin_n;
  uint32_t a[P];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t x = z.pin[j];
    if ((uint32_t)j >= m) {
      x = q[j];
#pragma unroll
      for (int k = 0; k < N - 1; ++k)
        if ((uint32_t)k < m) x += z.pin[k] <= x ? 1u : 0u;
    }
    a[j] = x;
  }
#pragma unroll
  for (int j = N; j < P; ++j) a[j] = 0xFFFFFFFFu;
  sort_network<P>(a);
  uint64_t r = 0;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    p[j] = a[j];
    r += binom[a[j] * (N + 1) + j + 1];
  }
  full_rank = r;
}

}  // namespace bote
