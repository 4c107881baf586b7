// bote_eval_topk.hip — the generic kernel's plain top-K instantiations
// (bote_eval.hpp; SCORE, MEAN, COV and MAX objectives: the fix-up and the
// fallback of every fast sweep): N = 2..16, base and extended keys.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                    \
  template __global__ void eval_kernel<NN, false, false>(EvalArgs); \
  template __global__ void eval_kernel<NN, false, true>(EvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_topk(uint32_t n, bool keys) {
  switch (n) {
#define FN_CASE(NN) \
  case NN: return keys ? (const void*)eval_kernel<NN, false, true> : (const void*)eval_kernel<NN, false, false>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
