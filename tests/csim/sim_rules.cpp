// TEST-ONLY: the device context's host rules -- csrc/ks_shape.h (which kernel sequence a key-switch chunk takes), csrc/device_tables.h (the
// tables a context uploads: k_k2n's lift classes among them) and csrc/behz_lists.h (the operand lists of the BEHZ multiply) -- behind sim_*
// entry points, so that the restatements of tests/launch_plan.py, tests/explicit_moduli.py and tests/bfv_multiply_plan.py are held to the
// product's own text on the CPU.  The headers need no HIP; the shape codes are KsShape's and KsKind's enumerators in order.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../reference-seal-backend_amd/csrc/behz_lists.h"
#include "../../reference-seal-backend_amd/csrc/device_tables.h"
#include "../../reference-seal-backend_amd/csrc/ks_shape.h"

using namespace he355;

namespace {
// limits: {latency max, LDS max, chunk}, the first two as he355_set_latency_max / he355_set_lds_max take them (2^64 - 1: the rule) and
// through the setters those calls use
KsLimits limits_of(uint64_t N, int K, const uint64_t *limits)
{
    KsLimits c;
    c.N = N; c.K = K;
    c.set_latency_max(limits[0]);
    c.set_lds_max(limits[1]);
    c.chunk = (size_t)limits[2];
    return c;
}
} // namespace

extern "C" {
// one cell of the rule: the environment's (scheme, logn1, K) and the context's (N, K, limits) are separate inputs, as in the product
int sim_ks_shape(int scheme, int logn1, int env_K, uint64_t N, int K, const uint64_t *limits, int L, uint64_t nc, int kind, int out_apart)
{
    return (int)ks_shape(KsDims{scheme, logn1, env_K}, limits_of(N, K, limits), L, nc, (KsKind)kind, out_apart != 0);
}
uint64_t sim_lat_limit(uint64_t N, int K, const uint64_t *limits) { return lat_limit(limits_of(N, K, limits)); }
uint64_t sim_lds_limit(int scheme, int logn1, int env_K, uint64_t N, int K, const uint64_t *limits, int L)
{
    return lds_limit(KsDims{scheme, logn1, env_K}, limits_of(N, K, limits), L);
}
// The whole rule over one chain in one call: L = 1 .. L_top, n = 1 .. n_max, the four kinds, out_apart 0 / 1.
//   shape [L_top][n_max][4][2], fuse [L_top][n_max], level_sum [n_chunks][L_top][n_max] (the limits' chunk replaced by chunks[k]),
//   lds_lim [L_top], lds_ok [L_top]; returns lat_limit
uint64_t sim_ks_scan(int scheme, int logn1, int env_K, uint64_t N, int K, const uint64_t *limits, int L_top, uint64_t n_max, const uint64_t *chunks,
                     size_t n_chunks, uint8_t *shape, uint8_t *fuse, uint8_t *level_sum, uint64_t *lds_lim, uint8_t *lds_ok)
{
    const KsDims e{scheme, logn1, env_K};
    const KsLimits c = limits_of(N, K, limits);
    for (int L = 1; L <= L_top; ++L) {
        lds_lim[L - 1] = lds_limit(e, c, L);
        lds_ok[L - 1] = ks_lds_supported(e, L) ? 1 : 0;
        for (uint64_t n = 1; n <= n_max; ++n) {
            const size_t at = (size_t)(L - 1) * n_max + (n - 1);
            fuse[at] = fuse_pays(e, n, L) ? 1 : 0;
            for (int kind = 0; kind < 4; ++kind)
                for (int apart = 0; apart < 2; ++apart) shape[(at * 4 + kind) * 2 + apart] = (uint8_t)ks_shape(e, c, L, n, (KsKind)kind, apart != 0);
            for (size_t k = 0; k < n_chunks; ++k) {
                KsLimits ck = c;
                ck.chunk = (size_t)chunks[k];
                level_sum[k * (size_t)L_top * n_max + at] = level_sum_pays(e, ck, L, n) ? 1 : 0;
            }
        }
    }
    return lat_limit(c);
}

// device_tables.h: k_k2n's class of one (digit prime, fp64-engine target) pair -- 0 general, 1 direct, 2 lift -- and the masks of a chain
// (p: a sim_params_* handle; direct, lift: K words)
int sim_k2_lift_class(uint64_t qj, uint64_t qt, int logn1) { return (int)k2_lift_class(qj, qt, logn1); }
void sim_k2_lift_masks(void *p, uint64_t *direct, uint64_t *lift)
{
    const Params &P = *(const Params *)p;
    std::vector<PrimeDev> pd(P.K);
    k2_lift_masks(P, pd.data());
    for (size_t j = 0; j < P.K; ++j) { direct[j] = pd[j].k2_direct; lift[j] = pd[j].k2_lift; }
}

// behz_lists.h: ix = {a_base, b_base, gs, b1, a_sg, a_si, b_sg, b_sj}; out = {G, I, J, na, n_cts, may_list, e_words, per_res, per_op, a_cts, b_cts}
void sim_behz_lists(const uint64_t *ix, uint64_t n, int L, size_t S, size_t N, uint64_t *out)
{
    Indexer3 x;
    x.a_base = ix[0]; x.b_base = ix[1]; x.gs = ix[2]; x.b1 = ix[3]; x.a_sg = ix[4]; x.a_si = ix[5]; x.b_sg = ix[6]; x.b_sj = ix[7];
    const BehzLists g = behz_lists(x, n, L, S, N);
    const uint64_t v[11] = {g.G, g.I, g.J, g.na, g.n_cts, g.may_list ? 1u : 0u, g.e_words, g.per_res, g.per_op, g.a_cts, g.b_cts};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
}
