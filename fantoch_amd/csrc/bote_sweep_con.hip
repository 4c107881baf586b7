// bote_sweep_con.hip — the fast sweep kernel's constrained instantiations
// (bote_sweep.hip CON; DESIGN.md §4 "Constrained sweeps"): every tail variant,
// N = 2..16, unpinned, and their lookup fast_fn_con.  A unit of its own so that
// it compiles beside bote_sweep.hip, whose other instantiations keep their code.
#define BOTE_FAST_CON_UNIT
#include "bote_sweep.hip"
