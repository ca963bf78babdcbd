// sim_cplx.cpp -- TEST-ONLY.  Runs the arithmetic of the complex scalar combination (csrc/cplx_core.h: the very functions the HIP kernel
// k_scalar_combine_cplx compiles -- the half picked by one bit of the NTT index, then poly_core.h's run rule and 128-bit sum), the residue
// rule of he355_ckks_complex_scalar_residues with the unit u of csrc/cplx_args.h, and the host client's complex codec on the CPU, so that
// tests/test_ckks_complex_core_cpu.py can hold them to Python integers and to the oracle without a GPU.  Built into tests/csim/_build; the
// product never contains it.
#include <cstring>

#include "../../reference-seal-backend_amd/csrc/client/he_client.h"
#include "../../reference-seal-backend_amd/csrc/cplx_args.h"
#include "../../reference-seal-backend_amd/csrc/cplx_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;
using client::Client;

extern "C" {

// k_scalar_combine_cplx on the n elements e0 .. e0 + n - 1 of one row under one prime: x [terms][n], a [terms][2] (the two scalars under
// this prime), cst [2] or null; run 0: the prime's own (bfv_mac_run)
void sim_cplx_combine(uint64_t n, int logN, uint64_t e0, uint64_t q, uint64_t terms, uint64_t run, const uint64_t *x, const uint64_t *a, const uint64_t *cst,
                      uint64_t *out)
{
    const ModU64 m = make_mod(q);
    if (!run) run = bfv_mac_run(q);
    for (uint64_t e = 0; e < n; ++e) {
        const u32 s = cplx_half(e0 + e, logN);
        out[e] = cplx_combine_sum(x + e, n, a, 2, 1, s, terms, cst ? cst[s] : 0, run, m);
    }
}
// he355_ckks_complex_scalar_residues under n primes with the units u; out [2][n]; returns 0 where the scalar is refused
int sim_cplx_scalar(double v_re, double v_im, const uint64_t *q, const uint64_t *u, int n, uint64_t *out)
{
    u128 ma, mb;
    bool na, nb;
    if (!cplx_scalar_integers(v_re, v_im, ma, na, mb, nb)) return 0;
    for (int i = 0; i < n; ++i) cplx_scalar_pair(ma, na, mb, nb, u[i], q[i], out[i], out[n + i]);
    return 1;
}
// he355_ckks_complex_unit / he355_ckks_complex_scalar_residues as the C ABI runs them (params: sim_params_create); 0: refused
int sim_cplx_units(void *params, int L, uint64_t *out)
{
    try {
        cplx_units(*(Params *)params, "sim", L, out);
        return 1;
    } catch (const std::invalid_argument &) {
        return 0;
    }
}
int sim_cplx_residues(void *params, int L, double v_re, double v_im, uint64_t *out)
{
    try {
        cplx_scalar_residues(*(Params *)params, "sim", L, v_re, v_im, out);
        return 1;
    } catch (const std::invalid_argument &) {
        return 0;
    }
}
// the host client's complex codec (c: simc_create): vals [n][2] -> out [Ltop][N]; plain [L][N] -> out [N/2][2]
void simc_ckks_encode_complex(void *c, const double *vals, size_t n, double scale, uint64_t *out)
{
    auto v = ((Client *)c)->ckks_encode_complex(vals, n, scale);
    std::memcpy(out, v.data(), v.size() * 8);
}
void simc_ckks_decode_complex(void *c, const uint64_t *plain, size_t L, double scale, double *out) { ((Client *)c)->ckks_decode_complex(plain, L, scale, out); }

} // extern "C"
