// bote_eval_full.hip — the generic kernel's full-output instantiations
// (bote_eval.hpp): N = 2..16, base and extended keys.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                   \
  template __global__ void eval_kernel<NN, true, false>(EvalArgs); \
  template __global__ void eval_kernel<NN, true, true>(EvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_full(uint32_t n, bool keys) {
  switch (n) {
#define FN_CASE(NN) \
  case NN: return keys ? (const void*)eval_kernel<NN, true, true> : (const void*)eval_kernel<NN, true, false>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
