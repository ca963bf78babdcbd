// sim_bsgs.cpp -- TEST-ONLY.  Runs the arithmetic of the baby-step/giant-step linear transform (csrc/bsgs_core.h: the very functions the HIP
// kernels k_hoist_rot_qp, k_bsgs_ident and k_bsgs_inner compile -- the folded P * c0 term, the identity baby's term, the accumulate, the
// run rule and the inner sum in one 128-bit accumulator) on the CPU, so that tests/test_linear_transform_bsgs_core_cpu.py can hold them to
// Python integers without a GPU.  Built into tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/he_params.h"
#include "../../reference-seal-backend_amd/csrc/bsgs_core.h"

using namespace he355;

extern "C" {

uint64_t sim_bsgs_p_mod(uint64_t P, uint64_t q) { return bsgs_p_mod(P, make_mod(q)); }
// k_hoist_rot_qp's polynomial 0 under a data prime before the permutation: s + P c0;  k_bsgs_ident: P c;  the giant accumulate: acc + v
void sim_bsgs_fold_c0(uint64_t n, uint64_t q, uint64_t P, const uint64_t *s, const uint64_t *c0, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    const uint64_t pmq = bsgs_p_mod(P, m);
    for (uint64_t e = 0; e < n; ++e) out[e] = bsgs_fold_c0(s[e], c0[e], pmq, m);
}
void sim_bsgs_ident(uint64_t n, uint64_t q, uint64_t P, const uint64_t *c, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    const uint64_t pmq = bsgs_p_mod(P, m);
    for (uint64_t e = 0; e < n; ++e) out[e] = bsgs_ident_term(c[e], pmq, m);
}
void sim_bsgs_acc(uint64_t n, uint64_t q, const uint64_t *acc, const uint64_t *v, uint64_t *out)
{
    for (uint64_t e = 0; e < n; ++e) out[e] = bsgs_acc(acc[e], v[e], q);
}
uint64_t sim_bsgs_run(const uint64_t *q, int n) { return bsgs_run(q, n); }
// k_bsgs_inner on n elements: t, p [terms][n]; run 0: the prime's own (bfv_mac_run)
void sim_bsgs_inner(uint64_t n, uint64_t q, uint64_t terms, uint64_t run, const uint64_t *t, const uint64_t *p, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    if (!run) run = bfv_mac_run(q);
    for (uint64_t e = 0; e < n; ++e) out[e] = bsgs_inner_sum(t + e, n, p + e, n, terms, run, m);
}
// how many folds the run rule makes over `terms` terms (the kernel's walk)
uint64_t sim_bsgs_folds(uint64_t terms, uint64_t run)
{
    uint64_t left = run, folds = 0;
    for (uint64_t k = 0; k < terms; ++k) {
        folds += bsgs_run_full(left, run);
        --left;
    }
    return folds;
}

} // extern "C"
