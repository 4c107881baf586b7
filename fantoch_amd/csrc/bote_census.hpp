// bote_census.hpp — census sweeps (DESIGN.md §4 "Census sweeps"): the second
// sink for a config's objective keys beside the block top-K (bote_device.hpp
// topk_step).  Per objective o and threshold t, the number of offered configs
// with (key_o, rank) < thr[o][t] in the lists' unsigned (key, rank) order.
//
// The sink shared by the two kernels that have a census variant
// (sweep_fast_kernel, bote_sweep.hip; eval_kernel, bote_eval.hpp).  In LDS:
//   thr  [n_obj][CENSUS_T] the launch's thresholds, ascending, padded with
//        all-ones records past T (no real record is at or above one: a rank is
//        below C(ns, n))
//   bin  [n_obj][CENSUS_T] u64: bin[o][j] counts the configs whose first
//        threshold above them is j; below[o][t] is the sum of bin[o][0 .. t]
// A lane takes one probe of the largest threshold (a uniform address), then a
// 4-step binary search and one 64-bit LDS add: no wave- or block-wide
// operation, so a lane without a config simply does nothing, and the counts do
// not depend on the order of the adds.  64-bit bins: a block's share of a
// launch is not bounded by 2^32.
#pragma once
#include "bote_kernels.hpp"

namespace bote {

// The kernels' arguments with the census fields at the end, as their
// launchers build them: the kernarg offsets of FastArgs and EvalArgs stay.
struct CensusFastArgs : FastArgs {
  CensusArgs cz;
};
struct CensusEvalArgs : EvalArgs {
  CensusArgs cz;
};

struct CensusLds {
  Rec* thr;
  unsigned long long* bin;
};

// The COV screen of finish_config (bote_fast.hpp) reads a threshold key as a
// double and drops a config whose V / S1^2 is above it.  That is the integer
// order only while the key is the bit pattern of a finite non-negative double:
// from +inf's pattern on (NaNs, negative doubles, all ones) every finite COV
// key is below the threshold although the comparison says otherwise, so such a
// threshold screens nothing (all ones is the screen's own "maybe").
constexpr uint64_t COV_KEY_INF = 0x7FF0000000000000ull;

// Every thread of the block; the caller's next barrier publishes it.  `screen`
// (null: none) receives per objective the key finish_config screens SCORE and
// COV keys with: the largest threshold's (a config that cannot beat the largest
// is below none).
__device__ inline void census_init(const CensusLds& c, Rec* screen, const CensusArgs& z, int n_obj,
                                   const uint32_t* obj_kind) {
  for (uint32_t i = threadIdx.x; i < (uint32_t)n_obj * CENSUS_T; i += blockDim.x) {
    const uint32_t o = i / CENSUS_T, t = i % CENSUS_T;
    c.thr[i] = t < z.T ? z.thr[o * z.T + t] : rec_max();
    c.bin[i] = 0;
  }
  if (screen && threadIdx.x < MAXOBJ) {
    Rec m = rec_max();
    if ((int)threadIdx.x < n_obj) {
      m = z.thr[threadIdx.x * z.T + z.T - 1];
      if (obj_kind[threadIdx.x] == OBJ_COV && m.key >= COV_KEY_INF) m.key = ~0ull;
    }
    screen[threadIdx.x] = m;
  }
}

// One config's keys into the bins.  ok[o] false: the lane offers nothing for
// objective o (no config, a deferred one, an invalid one for SCORE, or a key
// the screen dropped: it is below no threshold).
__device__ __forceinline__ void census_step(const CensusLds& c, int n_obj, uint32_t T, const uint64_t (&key)[MAXOBJ],
                                            const bool (&ok)[MAXOBJ], uint64_t rank) {
#pragma unroll
  for (int o = 0; o < MAXOBJ; ++o) {
    if (o >= n_obj) break;
    const Rec x{key[o], rank};
    const Rec* th = c.thr + o * CENSUS_T;
    if (ok[o] && rec_lt(x, th[T - 1])) {
      // the first threshold above x: thresholds 0 .. lo - 1 are at or below it
      // (entry T - 1 is above x and the padding is above everything, so the
      // probes, entries 0 .. CENSUS_T - 2, end at lo <= T - 1)
      uint32_t lo = 0;
#pragma unroll
      for (int st = CENSUS_T / 2; st >= 1; st >>= 1)
        if (!rec_lt(x, th[lo + st - 1])) lo += st;
      atomicAdd(&c.bin[o * CENSUS_T + lo], 1ull);
    }
  }
}

// After the block's last step and a barrier: the prefix sums of the bins leave
// by one 64-bit global add per count.
__device__ inline void census_flush(const CensusLds& c, const CensusArgs& z, int n_obj) {
  for (uint32_t i = threadIdx.x; i < (uint32_t)n_obj * z.T; i += blockDim.x) {
    const uint32_t o = i / z.T, t = i % z.T;
    unsigned long long s = 0;
    for (uint32_t j = 0; j <= t; ++j) s += c.bin[o * CENSUS_T + j];
    if (s) atomicAdd(&z.below[i], s);
  }
}

}  // namespace bote
