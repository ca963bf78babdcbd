// sim_bfv_select.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of a level of the BFV selection tree (csrc/bfv_gadget_core.h: the very
// functions the HIP kernels k_bfv_select_cols_fwd, k_bfv_select_spread, k_bfv_select_cols_inv and k_bfv_select_add compile -- the word whose
// digits the DIFF cut takes, its digit under an output prime, and the tail's add) on the CPU, so that tests/test_bfv_select_core_cpu.py can
// hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never contains it.
#include <cstddef>

#include "../../reference-seal-backend_amd/csrc/bfv_gadget_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// odd - even under the nodes' prime qi
uint64_t sim_bfvsel_diff(uint64_t odd, uint64_t even, uint64_t qi) { return bfv_select_diff(odd, even, qi); }
// out[g] = digit g < E of odd - even (width v) under output prime qj
void sim_bfvsel_diff_digits(uint64_t odd, uint64_t even, uint64_t qi, int E, int v, uint64_t qj, uint64_t *out)
{
    const ModU64 mj = make_mod(qj);
    for (int g = 0; g < E; ++g) out[g] = bfv_select_diff_digit(odd, even, qi, g, v, mj);
}
// the tail: the product's canonical word plus the even node's
uint64_t sim_bfvsel_add(uint64_t product, uint64_t even, uint64_t qi) { return bfv_select_add(product, even, qi); }

} // extern "C"
