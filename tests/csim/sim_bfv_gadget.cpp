// sim_bfv_gadget.cpp -- TEST-ONLY.  Runs the per-coefficient arithmetic of the BFV external product (csrc/bfv_gadget_core.h: the very functions
// the HIP kernels k_bfv_gadget_cols_fwd, k_bfv_gadget_spread, k_bfv_gadget_mac's caller and k_bfv_rgsw_plant compile -- the width-v gadget
// table, the uncentred digit under an output prime, the planted value, the index maps of the column pass and the pass split) on the CPU, so
// that tests/test_bfv_gadget_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never
// contains it.
#include <cstddef>

#include "../../reference-seal-backend_amd/csrc/bfv_gadget_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// the table of primes q[0 .. L-1] at digit width v: E[i], off[i] (L + 1 entries), bits[i]; returns E(L); *w = the width the table carries
uint32_t sim_bfvgad_table(const uint64_t *q, int L, int v, int *w, uint32_t *E, uint32_t *off, uint32_t *bits)
{
    const BfvDigitTab tab = bfv_gadget_table(q, L, v);
    *w = tab.w;
    for (int i = 0; i < L; ++i) { E[i] = tab.D[i]; off[i] = tab.off[i]; bits[i] = tab.bits[i]; }
    off[L] = tab.off[L];
    return tab.total;
}
int sim_bfvgad_width_ok(int v) { return bfv_gadget_width_ok(v) ? 1 : 0; }
// out[g] = digit g of x as the plain integer, g < E
void sim_bfvgad_digits(uint64_t x, int E, int v, uint64_t *out)
{
    for (int g = 0; g < E; ++g) out[g] = bfv_digit(x, g, v);
}
// digit g of x under output prime qj (Barrett constants made here as the product's tables make them)
uint64_t sim_bfvgad_digit_mod(uint64_t x, int g, int v, uint64_t qj)
{
    const ModU64 m = make_mod(qj);
    return bfv_gadget_digit(x, g, v, m);
}
// 2^(g v), the gadget element of digit g under its own prime
uint64_t sim_bfvgad_power(int g, int v) { return bfv_gadget_power(g, v); }
// what row (., i, g) of RGSW(m) adds at a coefficient m under its own prime qi
uint64_t sim_bfvgad_plant(uint64_t m, uint64_t t, int g, int v, uint64_t qi)
{
    const ModU64 mi = make_mod(qi);
    return bfv_gadget_plant(m, t, g, v, mi);
}
// digit polynomial pf of a batch of size-`size` ciphertexts: out = {residue polynomial, prime, digit}
void sim_bfvgad_src(const uint64_t *q, int L, int v, int size, uint64_t pf, uint64_t *out)
{
    const BfvDigitSrc s = bfv_gadget_src(bfv_gadget_table(q, L, v), size, pf);
    out[0] = s.poly; out[1] = (uint64_t)s.prime; out[2] = (uint64_t)s.digit;
}
// residue polynomial p of the batch -> the first digit polynomial the column pass's block writes
uint64_t sim_bfvgad_first(const uint64_t *q, int L, int v, int size, uint64_t p) { return bfv_gadget_first(bfv_gadget_table(q, L, v), size, p); }
// results per pass of an external product
uint64_t sim_bfvgad_pass(uint64_t terms, uint64_t n, uint64_t cap) { return bfv_gadget_pass(terms, n, cap); }

} // extern "C"
