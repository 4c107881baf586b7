// bote_eval_pctl.hip — the generic kernel's top-K instantiations with the
// percentile passes (bote_eval.hpp, EVAL_PCTL): N = 2..16, base and extended keys.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                               \
  template __global__ void eval_kernel<NN, false, false, EVAL_PCTL>(EvalArgs); \
  template __global__ void eval_kernel<NN, false, true, EVAL_PCTL>(EvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_pctl(uint32_t n, bool keys) {
  switch (n) {
#define FN_CASE(NN)                                                          \
  case NN:                                                                   \
    return keys ? (const void*)eval_kernel<NN, false, true, EVAL_PCTL>       \
                : (const void*)eval_kernel<NN, false, false, EVAL_PCTL>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
