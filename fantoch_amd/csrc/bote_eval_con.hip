// bote_eval_con.hip — the generic kernel's constrained instantiations
// (bote_eval.hpp CON; top-K, base keys, unpinned): N = 2..16, EVAL_PLAIN, and
// EVAL_MDTM for a sweep with a percentile or an MDTM entry among its objectives
// and constraints.
#include "bote_eval.hpp"

namespace bote {

#define INST(NN)                                                                                       \
  template __global__ void eval_kernel<NN, false, false, EVAL_PLAIN, false, false, true>(ConEvalArgs); \
  template __global__ void eval_kernel<NN, false, false, EVAL_MDTM, false, false, true>(ConEvalArgs);
BOTE_EVAL_SIZES(INST)

const void* eval_fn_con(uint32_t n, bool passes) {
  switch (n) {
#define FN_CASE(NN)                                                                                 \
  case NN:                                                                                          \
    return passes ? (const void*)eval_kernel<NN, false, false, EVAL_MDTM, false, false, true>       \
                  : (const void*)eval_kernel<NN, false, false, EVAL_PLAIN, false, false, true>;
    BOTE_EVAL_SIZES(FN_CASE)
    default: return nullptr;
  }
}

}  // namespace bote
