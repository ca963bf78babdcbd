// sim_bfv_digits.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of the BFV ciphertext decomposition (csrc/bfv_digits_core.h: the very
// functions the HIP kernels k_bfv_digits, k_bfv_undigits and k_bfv_digits_cols_fwd compile -- the digit table, a digit of a residue, the
// masked sum and its conditional subtraction) and the centred lift the fused kernel applies to a digit (csrc/bfv_level_core.h) on the CPU, so
// that tests/test_bfv_digits_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never
// contains it.
#include <cstring>

#include "../../reference-seal-backend_amd/csrc/bfv_digits_core.h"
#include "../../reference-seal-backend_amd/csrc/bfv_level_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// the table of primes q[0 .. L-1] and plain modulus t: D[i], off[i] (L + 1 entries), bits[i]; returns D(L); *w = the digit width
uint32_t sim_bfvdig_table(const uint64_t *q, int L, uint64_t t, int *w, uint32_t *D, uint32_t *off, uint32_t *bits)
{
    const BfvDigitTab tab = bfv_digit_table(q, L, t);
    *w = tab.w;
    for (int i = 0; i < L; ++i) { D[i] = tab.D[i]; off[i] = tab.off[i]; bits[i] = tab.bits[i]; }
    off[L] = tab.off[L];
    return tab.total;
}
// the bits compose keeps of digit g
int sim_bfvdig_keep(int g, int D, int b, int w) { return bfv_digit_keep(g, D, b, w); }
// the prime that owns digit index d < D(L), as the fused kernel finds it
int sim_bfvdig_prime(const uint64_t *q, int L, uint64_t t, uint32_t d) { return bfv_digit_prime(bfv_digit_table(q, L, t), d); }
// plaintext pf of a batch of size-`size` ciphertexts at level L: out = {residue polynomial of the ciphertext slab, prime, digit}, as the
// fused column pass finds its source
void sim_bfvdig_src(const uint64_t *q, int L, uint64_t t, int size, uint64_t pf, uint64_t *out)
{
    const BfvDigitSrc s = bfv_digit_src(bfv_digit_table(q, L, t), size, pf);
    out[0] = s.poly; out[1] = (uint64_t)s.prime; out[2] = (uint64_t)s.digit;
}
// out[g] = digit g of x, g < D
void sim_bfvdig_digits(uint64_t x, int D, int w, uint64_t *out)
{
    for (int g = 0; g < D; ++g) out[g] = bfv_digit(x, g, w);
}
// the residue k_bfv_undigits forms of D arbitrary 64-bit "digits" under a prime q of b bits
uint64_t sim_bfvdig_compose(const uint64_t *digits, int D, int b, int w, uint64_t q)
{
    u64 s = 0;
    for (int g = 0; g < D; ++g) s += bfv_undigit_term(digits[g], g, D, b, w);
    return bfv_undigit_finish(s, q);
}
// the centred lift of a digit under prime q (Barrett constants made here as the product's tables make them)
uint64_t sim_bfvdig_lift(uint64_t digit, uint64_t t, uint64_t q)
{
    ModU64 m = make_mod(q);
    return bfv_lift_centred(digit, t, m);
}

} // extern "C"
