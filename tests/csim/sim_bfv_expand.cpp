// sim_bfv_expand.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of the BFV monomial multiply and of the odd children of the
// query expansion (csrc/bfv_expand_core.h: the very functions the HIP kernel k_bfv_shift compiles -- the source index and sign of a shift,
// (2c - even) mod q) on the CPU, so that tests/test_bfv_expand_core_cpu.py can hold them to Python integers without a GPU.  Built into
// tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/bfv_expand_core.h"

using namespace he355;

extern "C" {

// idx[j], neg[j], j < N = 2^logN: where coefficient j of in * X^e comes from, and whether it is negated
void sim_bfvexp_shift_map(uint32_t e, int logN, uint32_t *idx, uint32_t *neg)
{
    for (uint32_t j = 0; j < ((uint32_t)1 << logN); ++j) {
        const BfvShiftSrc s = bfv_shift_src(j, e, logN);
        idx[j] = s.idx;
        neg[j] = s.neg;
    }
}
// out = in * X^e mod (X^N + 1, q) as a lane of the kernel computes each coefficient
void sim_bfvexp_shift(const uint64_t *in, uint32_t e, int logN, uint64_t q, uint64_t *out)
{
    for (uint32_t j = 0; j < ((uint32_t)1 << logN); ++j) {
        const BfvShiftSrc s = bfv_shift_src(j, e, logN);
        out[j] = bfv_shift_sign(in[s.idx], s.neg, q);
    }
}
uint64_t sim_bfvexp_odd(uint64_t c, uint64_t even, uint64_t q) { return bfv_expand_odd(c, even, q); }

} // extern "C"
