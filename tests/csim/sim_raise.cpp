// sim_raise.cpp -- TEST-ONLY.  Runs the arithmetic of the CKKS modulus raise (csrc/raise_core.h: the very functions the HIP kernels
// k_raise_lift and k_raise_cols compile -- the centred lift of a residue under q_0 into a target prime in the u64 engine's barrett form
// and in the fp64 engine's two forms -- and the host rule of the small-batch split) on the CPU, so that
// tests/test_ckks_mod_raise_core_cpu.py can hold them to Python integers without a GPU.  Built into tests/csim/_build; the product never
// contains it.
#include "../../reference-seal-backend_amd/csrc/he_params.h"
#include "../../reference-seal-backend_amd/csrc/raise_core.h"

using namespace he355;

extern "C" {

// the integer form: out[e] = centred(x[e]) mod qj, canonical
void sim_raise_lift_u64(uint64_t n, uint64_t q0, uint64_t qj, const uint64_t *x, uint64_t *out)
{
    const ModU64 mj = make_mod(qj);
    for (uint64_t e = 0; e < n; ++e) out[e] = raise_lift_u64(x[e], q0, mj);
}
// the fp64 engine's form (qj < 2^47), as k_raise_cols picks it from q0: out[e] = the canonical residue of the lazy value, lazy[e] its
// magnitude rounded up (the column pass's input range is the caller's to check); returns 1 for the wide form, 0 for the narrow one
int sim_raise_lift_f64(uint64_t n, uint64_t q0, uint64_t qj, const uint64_t *x, uint64_t *out, double *lazy)
{
    ArF64 ar;
    ar.q = (double)qj; ar.qinv = 1.0 / (double)qj; ar.ninv = 0; ar.ninv_i = 0;
    const double pow32 = (double)((((u64)1) << 32) % qj);
    const bool wide = (q0 >> 52) != 0, rc = raise_recentre(q0, qj);
    for (uint64_t e = 0; e < n; ++e) {
        const double v = wide ? raise_lift_f64_wide(ar, x[e], q0, pow32) : raise_lift_f64(ar, raise_centre_f64(x[e], q0), rc);
        out[e] = ar.to_canon(v);
        lazy[e] = v < 0 ? -v : v;
    }
    return wide ? 1 : 0;
}
int sim_raise_tsplit(uint64_t polys, int L_to, uint64_t cus) { return raise_tsplit(polys, L_to, cus); }

} // extern "C"
