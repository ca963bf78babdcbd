// sim_cheb.cpp -- TEST-ONLY.  Runs the per-lane arithmetic of the fused combine-and-rescale step (csrc/cheb_core.h: the very functions the
// HIP kernels k_scalar_combine_row and k_floor_rows_combine compile -- the E sums of a lane under the run rule, their reduction, and the
// floor step on the finished sum in the u64 engine's form of this build and in the fp64 engine's) on the CPU, so that
// tests/test_ckks_eval_mod_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never
// contains it.
#include "../../reference-seal-backend_amd/csrc/cheb_core.h"
#include "../../reference-seal-backend_amd/csrc/device_tables.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

namespace {
constexpr int kE = 4; // elements per simulated lane (the kernels: 2 and 16)
// tv [n]: the reduced sums of n elements (a multiple of kE), lane by lane; x [terms][n], a [terms], cst the constant's residue (0: none)
void lane_sums(uint64_t n, const ModU64 &m, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, uint64_t cst, uint64_t *tv)
{
    for (uint64_t e = 0; e < n; e += kE) {
        u128 s[kE];
        u64 left;
        cheb_sum_open(s, cst, left, run);
        for (uint64_t t = 0; t < terms; ++t) {
            u64 xv[kE];
            for (int r = 0; r < kE; ++r) xv[r] = x[t * n + e + r];
            cheb_sum_term(s, xv, a[t], left, run, m);
        }
        u64 v[kE];
        cheb_sum_close(s, m, v);
        for (int r = 0; r < kE; ++r) tv[e + r] = v[r];
    }
}
} // namespace

extern "C" {

int sim_cheb_form(void) { return HE355_U64_FOLD; }
// k_scalar_combine_row on n elements (a multiple of 4) under one prime; run 0: the prime's own (bfv_mac_run)
void sim_cheb_sums(uint64_t n, uint64_t q, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, uint64_t cst, uint64_t *out)
{
    lane_sums(n, make_mod(q), terms, run ? run : bfv_mac_run(q), x, a, cst, out);
}
// k_floor_rows_combine<ArU64> on n elements of a row of prime qi, the rescale dividing out qs: corr [n] the transformed correction as a lazy
// value below 4 qi.  (The fold build takes primes 2^60 - c only.)
void sim_cheb_fused_u64(uint64_t n, uint64_t qi, uint64_t qs, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, uint64_t cst, const uint64_t *corr,
                        uint64_t *out)
{
    const ModU64 m = make_mod(qi);
    ArU64 ar;
    ar.q = qi; ar.two_q = 2 * qi; ar.ninv = 0; ar.ninv_q = 0; ar.cr0 = m.cr0; ar.cr1 = m.cr1;
    const FloorConst fc = floor_const(qs, qi, ArU64::kFold);
    lane_sums(n, m, terms, run ? run : bfv_mac_run(qi), x, a, cst, out);
    for (uint64_t e = 0; e < n; ++e) out[e] = cheb_floor(ar, out[e], corr[e], fc);
}
// k_floor_rows_combine<ArF64> (qi below 2^50): corr [n] the transformed correction as the engine's centred double
void sim_cheb_fused_f64(uint64_t n, uint64_t qi, uint64_t qs, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, uint64_t cst, const double *corr,
                        uint64_t *out)
{
    const ModU64 m = make_mod(qi);
    ArF64 ar;
    ar.q = (double)qi; ar.qinv = 1.0 / (double)qi; ar.ninv = 0; ar.ninv_i = 0;
    const FloorConst fc = floor_const(qs, qi, false);
    lane_sums(n, m, terms, run ? run : bfv_mac_run(qi), x, a, cst, out);
    for (uint64_t e = 0; e < n; ++e) out[e] = cheb_floor(ar, out[e], corr[e], fc);
}

} // extern "C"
