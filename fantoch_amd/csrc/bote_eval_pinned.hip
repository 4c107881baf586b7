// bote_eval_pinned.hip — the generic kernel's pinned instantiations
// (bote_eval.hpp PIN, bote_pinned.hpp; top-K, base keys): N = 2..16,
// EVAL_PLAIN, and EVAL_MDTM for a sweep with a percentile or an MDTM objective.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                                         \
  template __global__ void eval_kernel<NN, false, false, EVAL_PLAIN, true>(PinEvalArgs); \
  template __global__ void eval_kernel<NN, false, false, EVAL_MDTM, true>(PinEvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_pinned(uint32_t n, bool passes) {
  switch (n) {
#define FN_CASE(NN)                                                                   \
  case NN:                                                                            \
    return passes ? (const void*)eval_kernel<NN, false, false, EVAL_MDTM, true>       \
                  : (const void*)eval_kernel<NN, false, false, EVAL_PLAIN, true>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
