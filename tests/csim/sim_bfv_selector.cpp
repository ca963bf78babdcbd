// sim_bfv_selector.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of the packed RGSW selectors (csrc/bfv_gadget_core.h: the very
// functions the HIP kernels k_bfv_selector_plant and the OWN forms of k_bfv_gadget_cols_fwd, k_bfv_gadget_spread and k_bfv_gadget_mac compile --
// (2^d)^(-1) mod q, the planted selector value and the destination row of a slot ciphertext) on the CPU, so that
// tests/test_bfv_selector_core_cpu.py can hold them to Python integers without a GPU.  The pass rule of he355_bfv_rgsw_from_bfv is
// bfv_gadget_pass unchanged (sim_bfvgad_pass, sim_bfv_gadget.cpp).  Built into tests/csim/_build; the product never contains it.
#include <cstddef>

#include "../../reference-seal-backend_amd/csrc/bfv_gadget_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// (2^d)^(-1) mod q, q odd
uint64_t sim_bfv_selector_inv_pow2(uint64_t q, int d) { return bfv_selector_inv_pow2(q, d); }
// what selector m (mod t) adds at the coefficient of digit g under the digit's own prime qi, for an expansion of depth d
uint64_t sim_bfv_selector_value(uint64_t m, uint64_t t, int g, int v, int d, uint64_t qi)
{
    const ModU64 mi = make_mod(qi);
    return bfv_selector_value(m, t, g, v, bfv_selector_inv_pow2(qi, d), mi);
}
// slot ciphertext c = (selector) E + f -> its row of the RGSW slab [.][2E][2][L][N], k = 0 or 1
uint64_t sim_bfv_selector_row(uint64_t c, uint32_t E, int k) { return bfv_selector_row(c, E, k); }

} // extern "C"
