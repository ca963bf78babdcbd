// TEST-ONLY: the device context's host rules -- csrc/ks_shape.h (which kernel sequence a key-switch chunk takes), csrc/ks_launch.h (which
// launches and grids the kernels of that sequence get), csrc/device_tables.h (the
// tables a context uploads: k_k2n's lift classes among them) and csrc/behz_lists.h (the operand lists of the BEHZ multiply) -- behind sim_*
// entry points, so that the restatements of tests/launch_plan.py, tests/explicit_moduli.py and tests/bfv_multiply_plan.py are held to the
// product's own text on the CPU.  The headers need no HIP; the shape codes are KsShape's and KsKind's enumerators in order.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../reference-seal-backend_amd/csrc/behz_lists.h"
#include "../../reference-seal-backend_amd/csrc/device_tables.h"
#include "../../reference-seal-backend_amd/csrc/ks_launch.h"
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

// ---- ks_launch.h ----------------------------------------------------------------------------------------------------------------------
// {kWaves, kBlock, kDualMaxBlocks, kDualMaxBlocksK3, kLatTargets, kLatSplit, kLatSplitU64}
void sim_kl_consts(int32_t *out)
{
    const int32_t v[7] = {kWaves, kBlock, (int32_t)kDualMaxBlocks, (int32_t)kDualMaxBlocksK3, kLatTargets, kLatSplit, kLatSplitU64};
    for (int i = 0; i < 7; ++i) out[i] = v[i];
}
// One launcher's plans over one chain in one call: L = 1 .. L_top, n = 1 .. n_max, every argument combination of `combos` [n_combos][8].
// A cell of out [L_top][n_max][n_combos][1 + 4 * 9]: the number of launches (-1: the header refused the arguments), then per launch
//   {form (0: the engine's or digit kind's own kernel, 1: the dual kernel, 2: k_k3_dual8), grid x, grid y, threads per block,
//    op-groups per block, the u64 side's op-groups per block (k_k3_dual8), waves, target split, engine (1 fp64, 2 u64; k_k2n: 1 narrow, 2 wide digits; 0 both)}.
// A level argument v of a combination: v >= 0 as it is, else L + 1 + v (-1: L, -2: L - 1).  The combinations per launcher:
//   0 launch_k1 {c2_only}   1 launch_k2 {tsplit}   2 launch_k3 {part, fuse (bit 1: with the rescale), tt_lo, tt_hi, n_split, n_split_u64,
//   group_size (0: not grouped, -1: n), sum_out}   3 launch_k3_combine {}   4 launch_floor_cols {polys per op, n_tgt, tsplit}
//   5 launch_floor_rows {n_tgt, n_src, tail_prime (-100: none)}   6 launch_rows_inv_select {polys per op}
void sim_kl_scan(int launcher, int scheme, int logn1, int K, const uint8_t *prime_f64, const uint64_t *prime_q, int L_top, uint64_t n_max,
                 const int32_t *combos, size_t n_combos, int32_t *out)
{
    const KsLaunchDims e{scheme, logn1, K, prime_f64, prime_q};
    for (int L = 1; L <= L_top; ++L)
        for (uint64_t n = 1; n <= n_max; ++n)
            for (size_t ci = 0; ci < n_combos; ++ci) {
                const int32_t *c = combos + ci * 8;
                int32_t *cell = out + (((size_t)(L - 1) * n_max + (n - 1)) * n_combos + ci) * 37, *row = cell + 1;
                const auto lv = [&](int32_t v) { return v >= 0 ? (int)v : L + 1 + (int)v; };
                const auto put = [&](int form, unsigned gx, unsigned gy, int threads, int ogpb = 0, int ogpb_u64 = 0, int waves = 0, int ts = 0, int engine = 0) {
                    const int32_t v[9] = {form, (int32_t)gx, (int32_t)gy, threads, ogpb, ogpb_u64, waves, ts, engine};
                    for (int i = 0; i < 9; ++i) *row++ = v[i];
                };
                try {
                    if (launcher == 0) {
                        const K1Geometry G = k1_geometry(e, L, n, c[0] != 0);
                        if (G.dual) put(1, G.dual_grid[0] + G.dual_grid[1], 1, kBlock);
                        else
                            for (int p = 0; p < 2; ++p)
                                if (G.grid[p]) put(0, G.grid[p], 1, kBlock, 0, 0, 0, 0, p + 1);
                    } else if (launcher == 1) {
                        const K2Geometry G = k2_geometry(e, L, n, c[0]);
                        if (G.dual) put(1, G.gx[0] + G.gx[1], (unsigned)G.ts[0], kBlock, 0, 0, 0, G.ts[0]);
                        else
                            for (int w = 0; w < 2; ++w)
                                if (G.gx[w]) put(0, G.gx[w], (unsigned)G.ts[w], kBlock, 0, 0, 0, G.ts[w], w + 1);
                    } else if (launcher == 2) {
                        K3Request r;
                        r.L = L; r.n_ops = n; r.part = (K3Part)c[0]; r.fuse = (c[1] & 1) != 0; r.rescale = (c[1] & 2) != 0;
                        r.tt_lo = lv(c[2]); r.tt_hi = lv(c[3]); r.n_split = c[4]; r.n_split_u64 = c[5];
                        r.grouped = c[6] != 0; r.group_size = c[6] < 0 ? (u32)n : (u32)c[6]; r.sum_out = c[7] != 0;
                        const K3Geometry G = k3_geometry(e, r);
                        const K3Pass *P = G.pend;
                        if (G.n_pend == 2 && G.form == K3Form::Dual) put(1, P[0].g + P[1].g, (unsigned)std::max(P[0].n_split, P[1].n_split), 64, 0, 0, 1);
                        else if (G.n_pend == 2 && G.form == K3Form::Dual8) put(2, P[0].g + P[1].g, 1, 512, (int)P[0].og_per_block, (int)P[1].og_per_block, P[1].waves);
                        else
                            for (int i = 0; i < G.n_pend; ++i)
                                put(0, P[i].g, (unsigned)P[i].n_split, 64 * P[i].waves, (int)P[i].og_per_block, 0, P[i].waves, 0, P[i].f64 ? 1 : 2);
                    } else if (launcher == 3) {
                        put(0, k3_combine_grid(e, L, n), 1, kBlock);
                    } else if (launcher == 4) {
                        const FloorColsGrid g = floor_cols_grid(n * (uint64_t)c[0], c[2]);
                        if (lv(c[1]) > 0) put(0, g.x, g.y, kBlock, 0, 0, 0, (int)g.y); // (launch_floor_cols: no targets, no launch)
                    } else if (launcher == 5) {
                        const FloorRowsGeometry G = floor_rows_geometry(e, n, lv(c[0]), c[1], c[2] == -100 ? -1 : lv(c[2]));
                        if (G.dual) put(1, G.g[0] + G.g[2], 1, kBlock);
                        else
                            for (int p = 0; p < 4; ++p)
                                if (G.g[p]) put(0, G.g[p], 1, kBlock, 0, 0, 0, 0, p < 2 ? 1 : 2);
                    } else {
                        put(0, rows_inv_select_grid(e, n * (uint64_t)c[0]), 1, kBlock);
                    }
                    cell[0] = (int32_t)((row - cell - 1) / 9);
                } catch (const std::runtime_error &) {
                    cell[0] = -1;
                }
            }
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
