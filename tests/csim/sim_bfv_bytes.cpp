// sim_bfv_bytes.cpp -- TEST-ONLY.  Runs the arithmetic of the PIR database codec (csrc/bfv_bytes_core.h: the very functions the HIP kernels
// k_bfv_unpack, k_bfv_pack and k_bfv_bytes_cols_fwd compile -- a field cut out of aligned words at any byte address, one packed output word,
// the field count) and the centred lift the fused kernel applies to a field (csrc/bfv_level_core.h) on the CPU, so that
// tests/test_bfv_bytes_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never contains it.
#include <cstring>

#include "../../reference-seal-backend_amd/csrc/bfv_bytes_core.h"
#include "../../reference-seal-backend_amd/csrc/bfv_level_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// Bmax of N fields of w bits
uint64_t sim_bfvbytes_max(uint64_t N, int w) { return bfv_bytes_max(N, w); }
// how many coefficients of a B-byte plaintext can be non-zero
uint64_t sim_bfvbytes_fields(uint64_t B, int w) { return bfv_bytes_fields(B, w); }
// the words pack writes per plaintext
uint64_t sim_bfvbytes_words(uint64_t B) { return bfv_bytes_words(B); }
// out[e] = coefficient e < N of the B bytes at `bytes` (any address), as the kernels cut it
void sim_bfvbytes_unpack(const void *bytes, uint64_t B, int w, uint64_t N, uint64_t *out)
{
    const BfvByteSrc s = bfv_bytes_src(bytes, B);
    for (uint64_t e = 0; e < N; ++e) out[e] = bfv_bytes_field(s, e, w);
}
// output word k of the plaintext coef[0 .. N-1] (any 64-bit words)
uint64_t sim_bfvbytes_pack_word(const uint64_t *coef, uint64_t N, uint64_t k, uint64_t B, int w) { return bfv_bytes_pack_word(coef, N, k, B, w); }
// the centred lift of a field under prime q (Barrett constants made here as the product's tables make them)
uint64_t sim_bfvbytes_lift(uint64_t field, uint64_t t, uint64_t q)
{
    ModU64 m = make_mod(q);
    return bfv_lift_centred(field, t, m);
}

} // extern "C"
