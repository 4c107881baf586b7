// bote_eval_mdtm.hip — the generic kernel's top-K instantiations with the
// percentile and the MDTM passes (bote_eval.hpp, EVAL_MDTM): N = 2..16, base
// and extended keys.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                               \
  template __global__ void eval_kernel<NN, false, false, EVAL_MDTM>(EvalArgs); \
  template __global__ void eval_kernel<NN, false, true, EVAL_MDTM>(EvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_mdtm(uint32_t n, bool keys) {
  switch (n) {
#define FN_CASE(NN)                                                          \
  case NN:                                                                   \
    return keys ? (const void*)eval_kernel<NN, false, true, EVAL_MDTM>       \
                : (const void*)eval_kernel<NN, false, false, EVAL_MDTM>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
