// bote_eval_census.hip — the generic kernel's census instantiations
// (bote_eval.hpp CENSUS, bote_census.hpp; base keys, ranks and rank lists):
// N = 2..16, EVAL_PLAIN, and EVAL_MDTM for a census with a percentile or an
// MDTM objective, and the two small kernels around a census launch: the one
// that starts it and the one that picks its result on the device.
#include "bote_eval.hpp"
#include "bote_launch.hpp"

namespace bote {

#define INST(NN)                                                                                   \
  template __global__ void eval_kernel<NN, false, false, EVAL_PLAIN, false, true>(CensusEvalArgs); \
  template __global__ void eval_kernel<NN, false, false, EVAL_MDTM, false, true>(CensusEvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_census(uint32_t n, bool passes) {
  switch (n) {
#define FN_CASE(NN)                                                                          \
  case NN:                                                                                   \
    return passes ? (const void*)eval_kernel<NN, false, false, EVAL_MDTM, false, true>       \
                  : (const void*)eval_kernel<NN, false, false, EVAL_PLAIN, false, true>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

// The start of a census launch: the thresholds, which travel in the kernel's
// own arguments (no host buffer has to outlive the call), into their device
// table, and the launch's counts, valid counts and deferred count zeroed.
struct CensusThresholds {
  Rec r[MAXOBJ * CENSUS_T];
};
__global__ void __launch_bounds__(MAXOBJ* CENSUS_T)
    census_begin_kernel(CensusThresholds h, uint32_t n, Rec* thr, unsigned long long* below,
                        unsigned long long* below_alt, unsigned long long* counters, unsigned long long* counters_alt,
                        unsigned long long* qcount) {
  const uint32_t i = threadIdx.x;
  if (i < n) {
    thr[i] = h.r[i];
    below[i] = 0;
    if (below_alt) below_alt[i] = 0;
  }
  if (i < 2) {
    counters[i] = 0;
    if (counters_alt) counters_alt[i] = 0;
  }
  if (i == 0 && qcount) *qcount = 0;
}

hipError_t launch_census_begin(const Rec* host_thr, uint32_t n, Rec* thr, unsigned long long* below,
                               unsigned long long* below_alt, unsigned long long* counters,
                               unsigned long long* counters_alt, unsigned long long* qcount, hipStream_t st) {
  if ((n && !host_thr) || n > (uint32_t)MAXOBJ * CENSUS_T || !thr || !below || !counters) return hipErrorInvalidValue;
  CensusThresholds h{};
  for (uint32_t i = 0; i < n; ++i) h.r[i] = host_thr[i];
  hipLaunchKernelGGL(census_begin_kernel, dim3(1), dim3(MAXOBJ * CENSUS_T), 0, st, h, n, thr, below, below_alt, counters,
                     counters_alt, qcount);
  return hipGetLastError();
}

// A census's result: the fast pass's counts with its fix-up's, or the
// fallback's when the deferred queue overflowed (*sel > cap), chosen here so
// that a launch needs no host round trip.  One block; n <= MAXOBJ * CENSUS_T.
__global__ void __launch_bounds__(MAXOBJ* CENSUS_T + 64)
    census_pick_kernel(const unsigned long long* src, const unsigned long long* alt, uint32_t n,
                       const unsigned long long* csrc, const unsigned long long* calt, const unsigned long long* sel,
                       uint64_t cap, uint64_t* dst) {
  const bool over = sel && *sel > cap;
  const uint32_t i = threadIdx.x;
  if (i < n) dst[i] = over ? alt[i] : src[i];
  if (i == n) dst[n] = over ? calt[0] : csrc[0];
}

hipError_t launch_census_pick(const unsigned long long* src, const unsigned long long* alt, uint32_t n,
                              const unsigned long long* csrc, const unsigned long long* calt,
                              const unsigned long long* sel, uint64_t cap, uint64_t* dst, hipStream_t st) {
  if (!src || !csrc || !dst || n > (uint32_t)MAXOBJ * CENSUS_T || (sel && (!alt || !calt))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(census_pick_kernel, dim3(1), dim3(MAXOBJ * CENSUS_T + 64), 0, st, src, alt, n, csrc, calt, sel, cap,
                     dst);
  return hipGetLastError();
}

}  // namespace bote
