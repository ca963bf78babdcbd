// sim_poly.cpp -- TEST-ONLY.  Runs the arithmetic of the scalar combination (csrc/poly_core.h: the very functions the HIP kernel
// k_scalar_combine compiles -- the run rule with the constant as the first run's first term, the one 128-bit sum and its reduction) and
// the scalar-residue rule of he355_ckks_scalar_residues on the CPU, so that tests/test_ckks_eval_poly_core_cpu.py can hold them to Python
// integers without a GPU.  Built into tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/he_params.h"
#include "../../reference-seal-backend_amd/csrc/poly_core.h"

using namespace he355;

extern "C" {

uint64_t sim_poly_run(const uint64_t *q, int n) { return poly_run(q, n); }
// k_scalar_combine on n elements under one prime: x [terms][n], a [terms] (the scalar under this prime), cst the constant (0: none);
// run 0: the prime's own (bfv_mac_run)
void sim_poly_combine(uint64_t n, uint64_t q, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, uint64_t cst, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    if (!run) run = bfv_mac_run(q);
    for (uint64_t e = 0; e < n; ++e) out[e] = poly_combine_sum(x + e, n, a, 1, terms, cst, run, m);
}
// he355_ckks_scalar_residues under n primes; returns 0 where the scalar is refused
int sim_poly_scalar(double v, const uint64_t *q, int n, uint64_t *out)
{
    u128 mag;
    bool neg;
    if (!poly_scalar_integer(v, mag, neg)) return 0;
    for (int i = 0; i < n; ++i) out[i] = poly_scalar_residue(mag, neg, q[i]);
    return 1;
}

} // extern "C"
