// sim_bfv_merge.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of a level of the BFV ciphertext merge (csrc/bfv_merge_core.h and the
// shift map of csrc/bfv_expand_core.h: the very functions the HIP kernel k_bfv_merge compiles) on the CPU, so that
// tests/test_bfv_merge_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never
// contains it.
#include "../../reference-seal-backend_amd/csrc/bfv_merge_core.h"

using namespace he355;

extern "C" {

// S = even + X^s odd, D = even - X^s odd mod (X^N + 1, q), N = 2^logN, as a lane of the kernel computes each coefficient
void sim_bfvmerge_level(const uint64_t *even, const uint64_t *odd, uint32_t s, int logN, uint64_t q, uint64_t *S, uint64_t *D)
{
    for (uint32_t j = 0; j < ((uint32_t)1 << logN); ++j) {
        const BfvShiftSrc src = bfv_shift_src(j, s, logN);
        const BfvMergePair z = bfv_merge_pair(even[j], odd[src.idx], src.neg, q);
        S[j] = z.s;
        D[j] = z.d;
    }
}
// one coefficient: out[0] = S, out[1] = D
void sim_bfvmerge_pair(uint64_t even, uint64_t odd, uint32_t neg, uint64_t q, uint64_t *out)
{
    const BfvMergePair z = bfv_merge_pair(even, odd, neg, q);
    out[0] = z.s;
    out[1] = z.d;
}

} // extern "C"
