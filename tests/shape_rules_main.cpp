// shape_rules_main.cpp -- TEST-ONLY, stand-alone.  Walks the device context's host rules -- csrc/ks_shape.h, csrc/ks_launch.h,
// csrc/device_tables.h and csrc/behz_lists.h -- at their edges: batches of 0, 1, 2^32 and 2^63, L = 1 and L_top, logn1 = 0 and 5 (N = 1024 and 32768), a one-prime
// chain (K = 1), each limit set to 0 (the shape is never taken), to 2^64 - 1 (the rule applies again) and to 2^64 - 2, indexers with gs >= n and
// with gs that does not divide n; the launch geometry at no ops, L = 1, chains of one engine, kMaxPrimes primes with every list full, the
// level sum's and the other geometry refusals (caught, their texts checked) and the largest grid of the case table -- compiled with -fsanitize=address,undefined (tests/test_launch_plan_cpu.py).  The rules shift by logn1,
// multiply batch sizes the caller chose and index tables by prime: none of it may overflow a signed type, shift out of range, divide by zero or
// reach outside a vector (unsigned wrap at an absurd batch is the product's behaviour and stays).  Where a value can be checked in a line it
// is: the tables' inverses invert, the masks name fp64-engine targets only, the lists of a batch hold every operand a result reads.
// Prints "shape_rules ok" and exits 0, or names the first case that went the other way.
#include <cstdio>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/behz_lists.h"
#include "../reference-seal-backend_amd/csrc/device_tables.h"
#include "../reference-seal-backend_amd/csrc/ks_launch.h"
#include "../reference-seal-backend_amd/csrc/ks_shape.h"
#include "args_main_common.h"

using namespace he355;

static void must(bool ok, const char *what)
{
    if (!ok) throw std::invalid_argument(std::string("wrong rule: ") + what);
}
static u64 mw_mod(const u64 *x, int words, u64 q)
{
    u64 r = 0;
    for (int i = words - 1; i >= 0; --i) r = (u64)((((u128)r << 64) | x[i]) % q);
    return r;
}
static const u64 kBatches[] = {0, 1, (u64)1 << 32, (u64)1 << 63};

static void walk_shapes(const Params &P)
{
    const int Ltop = (int)P.Ltop;
    for (int scheme : {kSchemeBFV, kSchemeCKKS})
        for (int lat = 0; lat < 3; ++lat)
            for (int lds = 0; lds < 3; ++lds) {
                const KsDims e{scheme, P.logn1, (int)P.K};
                KsLimits c;
                c.N = P.N; c.K = (int)P.K;
                c.set_latency_max(lat == 0 ? ~(u64)0 : lat == 1 ? 0 : ~(u64)0 - 1); // the setters he355_set_latency_max / he355_set_lds_max use
                c.set_lds_max(lds == 0 ? ~(u64)0 : lds == 1 ? 0 : ~(u64)0 - 1);
                must(c.lat_auto == (lat == 0) && c.lds_auto == (lds == 0) && (lat != 0 || c.lat_max == 0) && (lds != 0 || c.lds_max == 0), "2^64 - 1: back to the rule");
                for (int L : {1, Ltop})
                    for (u64 n : kBatches)
                        for (size_t chunk : {(size_t)1, (size_t)1024, ~(size_t)0}) {
                            c.chunk = chunk;
                            (void)fuse_pays(e, n, L);
                            (void)level_sum_pays(e, c, L, n);
                            for (int kind = 0; kind < 4; ++kind)
                                for (int apart = 0; apart < 2; ++apart) {
                                    const KsShape s = ks_shape(e, c, L, n, (KsKind)kind, apart != 0);
                                    must((s == KsShape::BfvCoeff) == (scheme != kSchemeCKKS), "BfvCoeff is the BFV environment's shape, and its only one");
                                    if (kind == (int)KsKind::Grouped) must(s != KsShape::Lds && s != KsShape::Latency, "grouped: fused or unfused");
                                    if (lat == 1 && n) must(s != KsShape::Latency, "limit 0: never the latency shape");
                                    if (lds == 1 && n) must(s != KsShape::Lds, "limit 0: never the ring-in-LDS shape");
                                    if (P.K < 2) must(s != KsShape::Lds && s != KsShape::Latency && s != KsShape::Fused, "one prime: no key switch shape but unfused");
                                }
                        }
                must(lat_limit(c) == (lat == 0 ? std::min<u64>(12, ((u64)1 << 17) / P.N) : lat == 1 ? 0 : ~(u64)0 - 1), "lat_limit");
                must(lds_limit(e, c, 1) == (lds == 0 ? (u64)192 << (3 - std::min(3, P.logn1)) : lds == 1 ? 0 : ~(u64)0 - 1), "lds_limit");
                must(ks_lds_supported(e, Ltop) == (P.logn1 <= 3 && P.K >= 2 && Ltop <= 6), "ks_lds_supported");
            }
    for (int L : {1, Ltop}) {
        must(scratch_words_per_op(P.N, L) == (size_t)(L + 12) * L * P.N + 7 * P.N, "scratch words");
        must(scratch_words_per_op(P.N, L) - 2 * (size_t)L * P.N >= (size_t)(L + 2) * 2 * L * P.N || L > 6, "the LDS shape's partial products fit behind c01");
    }
    must(halve_until_fit(1000, [](size_t k) { return k <= 7; }) == 4 && halve_until_fit(1, [](size_t) { return false; }) == 0 &&
             halve_until_fit(5, [](size_t k) { return k == 1; }) == 1, "halve_until_fit");
}

// ks_launch.h over one set of dimensions: every launcher's geometry at level L for n ops.  The lists of the two engines (digit kinds,
// passes) partition their range, a grid has a block for every job, and a k_k3 grid is whole 8-tile groups.
static void walk_geometry(const KsLaunchDims &e, int L, u64 n)
{
    for (int c2 = 0; c2 < 2; ++c2) {
        const K1Geometry G = k1_geometry(e, L, n, c2 != 0);
        must(G.i_list[0].n + G.i_list[1].n == L, "k_k1: every residue on one engine");
        for (int p = 0; p < 2; ++p) must((u64)G.grid[p] * kWaves >= (n * G.i_list[p].n) << e.logn1 && (G.grid[p] != 0) == (G.dual_grid[p] != 0), "k_k1: a wave per row job");
        must(!G.dual || (!c2 && G.grid[0] && G.grid[1] && (n <= 8 || G.dual_grid[0] + G.dual_grid[1] <= kDualMaxBlocks)), "k_k1_dual: both engines, small grids");
    }
    for (int tsplit : {1, kLatTargets}) {
        const K2Geometry G = k2_geometry(e, L, n, tsplit);
        must(G.dig_list[0].n + G.dig_list[1].n == L && G.gx[0] + G.gx[1] == (unsigned)(n * L * 4), "k_k2n: every digit of one kind");
        for (int w = 0; w < 2; ++w) must(!G.gx[w] || (tsplit > 1 ? G.ts[w] == tsplit : G.ts[w] == 1 || G.ts[w] == 2 || G.ts[w] == 4), "k_k2n: target split");
        must(!G.dual || (G.gx[0] && G.gx[1]), "k_k2n_dual: both digit kinds");
    }
    must(f64_mask(e) >> (e.K < 64 ? e.K : 63) <= 1, "f64_mask: the chain's primes only");
    for (int part = 0; part < 3; ++part)
        for (int form = 0; form < 4; ++form) { // unfused; fused over [0, L); grouped with the level sum; the latency splits
            K3Request r;
            r.L = L; r.n_ops = n; r.part = (K3Part)part;
            if (form == 1 || form == 2) { r.fuse = true; r.tt_lo = 0; r.tt_hi = L; }
            if (form == 2) { r.grouped = true; r.group_size = 8; r.sum_out = true; }
            if (form == 3) { r.n_split = kLatSplit; r.n_split_u64 = kLatSplitU64; }
            if (form == 2 && n % 8) continue;
            const K3Geometry G = k3_geometry(e, r);
            int tiles = 0;
            for (int i = 0; i < G.n_pend; ++i) {
                const K3Pass &P = G.pend[i];
                tiles += P.tt_list.n;
                must(P.tt_list.n > 0 && P.g > 0 && (P.waves == 1 || P.g % 8 == 0), "k_k3: whole 8-tile groups");
                must(P.waves == (form == 3 ? 1 : P.waves) && (P.waves == 1 || P.waves == 8 || (P.waves == 4 && !P.f64)), "k_k3: waves");
                const u64 tiles8 = ((((u64)P.tt_list.n << e.logn1) + 7) / 8) * 8;
                if (!G.level_sum) must((u64)P.g / tiles8 * P.og_per_block * P.waves >= n && P.og_stride == 1, "k_k3: every op in an op-group of a block");
                else must((u64)P.g / tiles8 == 1 && (u64)P.og_per_block * 8 == n && P.og_stride == 1, "k_k3: the level sum walks the groups");
                for (int k = 0; k < P.tt_list.n; ++k) must(P.tt_list.at[k] <= L && P.q_slot[k] <= G.n_q, "k_k3: tiles and quotient slots");
            }
            const int want = n == 0 ? 0 : r.fuse ? (part == K3_DATA_ONLY ? L : part == K3_ALL ? L : 0) : part == K3_ALL ? L + 1 : part == K3_SPECIAL_ONLY ? 1 : L;
            must(tiles == want, "k_k3: every tile of the part on one engine");
            must(G.form == K3Form::Separate || G.n_pend == 2, "k_k3_dual / k_k3_dual8: both engines");
        }
    must((u64)k3_combine_grid(e, L, n) * kWaves >= (n * 2 * (u64)(L + 1)) << e.logn1, "k_k3_combine");
    must(floor_cols_grid(n * 2, 1).y == 1 && floor_cols_grid(n * 2, kLatTargets).y == (unsigned)kLatTargets && floor_cols_grid(n * 2, 0).x == (unsigned)(n * 8), "k_floor_colsn");
    for (int n_tgt : {L, L - 1})
        for (int n_src : {2, 3})
            for (int tail : {-1, n_tgt - 1}) {
                const FloorRowsGeometry G = floor_rows_geometry(e, n, n_tgt, n_src, tail);
                must(G.jobs_per_block >= (u32)kWaves && G.jobs_per_block <= 8u * kWaves, "k_floor_rows: jobs per block");
                must(G.i_list[0].n + G.i_list[1].n + G.i_list[2].n + G.i_list[3].n == n_tgt && G.i_list[1].n + G.i_list[3].n == (tail >= 0 ? 1 : 0), "k_floor_rows: every target in one pass");
                for (int p = 0; p < 4; ++p) must((u64)G.g[p] * G.jobs_per_block >= (n * n_src * G.i_list[p].n) << e.logn1, "k_floor_rows: a block for every job");
                must(!G.dual || (tail < 0 && G.g[0] && G.g[2]), "k_floor_rows_dual: both engines, no tail prime");
            }
    must((u64)rows_inv_select_grid(e, n * 2) * kWaves >= (n * 2) << e.logn1, "k_rows_inv_select");
}
static void refused(const char *text, const KsLaunchDims &e, const K3Request &r)
{
    try {
        (void)k3_geometry(e, r);
    } catch (const std::runtime_error &x) {
        must(std::string(x.what()) == text, text);
        return;
    }
    must(false, text);
}
static void walk_launches(const Params &P)
{
    std::vector<unsigned char> f64(P.K);
    std::vector<u64> q(P.K);
    for (size_t i = 0; i < P.K; ++i) { f64[i] = P.primes[i].f64 ? 1 : 0; q[i] = P.primes[i].q; }
    const KsLaunchDims e{kSchemeCKKS, P.logn1, (int)P.K, f64.data(), q.data()};
    for (int L : {1, (int)P.Ltop})
        for (u64 n : {(u64)0, (u64)1, (u64)7, (u64)8, (u64)64, (u64)512}) walk_geometry(e, L, n);
    // the refusals that are part of the geometry
    if (P.K >= 2) {
        const int L = (int)P.Ltop;
        K3Request r;
        r.L = L; r.n_ops = 64; r.part = K3_DATA_ONLY; r.fuse = true; r.tt_lo = 0; r.tt_hi = L; r.grouped = true; r.sum_out = true;
        const char *sum = "level sum in k_k3: fused 8-wave launches over whole groups of a multiple of eight ciphertexts";
        r.group_size = 12; refused(sum, e, r);                      // not a multiple of eight
        r.group_size = 24; refused(sum, e, r);                      // not whole groups
        r.group_size = 16; r.g_op_offset = 8; refused(sum, e, r);   // the launch does not start at a group
        r.g_op_offset = 16; GOOD("level sum", (void)k3_geometry(e, r));
        r.n_split = 2; refused("digit-split K3: unfused launches with a partial-sum buffer only", e, r);
        r.n_ops = 0; refused("digit-split K3: unfused launches with a partial-sum buffer only", e, r); // (refused before the empty launch returns)
        K3Request t;
        t.L = L; t.n_ops = 1; t.part = K3_DATA_ONLY; t.fuse = true; t.rescale = true; t.tt_lo = 0; t.tt_hi = L;
        refused("fused rescale: only primes below the one divided out", e, t);
        t.tt_hi = L - 1; GOOD("fused rescale", (void)k3_geometry(e, t));
        t.n_ops = 0; t.tt_hi = L; GOOD("no ops, no refusal of the range", must(k3_geometry(e, t).n_pend == 0, "no ops: no launch"));
    }
}
// kMaxPrimes primes: every list full -- all on the fp64 engine, all on the u64 engine (narrow and wide digits), and alternating
static void walk_full_lists()
{
    for (int kind = 0; kind < 4; ++kind) {
        unsigned char f64[kMaxPrimes];
        u64 q[kMaxPrimes];
        for (int i = 0; i < kMaxPrimes; ++i) {
            f64[i] = kind == 0 ? 1 : kind == 3 ? i & 1 : 0;
            q[i] = f64[i] ? (u64)1 << 44 : kind == 1 ? (u64)1 << 49 : (u64)1 << 59;
        }
        for (int logn1 : {0, 5}) {
            const KsLaunchDims e{kSchemeCKKS, logn1, kMaxPrimes, f64, q};
            for (u64 n : {(u64)1, (u64)512}) walk_geometry(e, kMaxPrimes - 1, n);
            must(k1_geometry(e, kMaxPrimes, 1, false).i_list[kind == 0 ? 0 : 1].n == (kind == 3 ? kMaxPrimes / 2 : kMaxPrimes), "k_k1: a full list");
            must(floor_rows_geometry(e, 1, kMaxPrimes, 2, -1).i_list[kind == 0 ? 0 : 2].n == (kind == 3 ? kMaxPrimes / 2 : kMaxPrimes), "k_floor_rows: a full list");
            K3Request r;
            r.L = kMaxPrimes - 1; r.n_ops = 1;
            must(k3_geometry(e, r).pend[0].tt_list.n == (kind == 3 ? kMaxPrimes / 2 : kMaxPrimes), "k_k3: a full list");
            must(k2_geometry(e, kMaxPrimes, 1, 1).dig_list[kind == 2 ? 1 : 0].n == (kind == 3 ? kMaxPrimes / 2 : kMaxPrimes), "k_k2n: a full list");
        }
    }
}

static void walk_tables(const Params &P)
{
    std::vector<PrimeDev> pd(P.K);
    for (size_t i = 0; i < P.K; ++i) {
        prime_dev_fill(pd[i], P.primes[i], P.N);
        must(pd[i].q == P.primes[i].q && pd[i].fwd == nullptr && pd[i].inv == nullptr && (pd[i].f64 != 0) == P.primes[i].f64, "PrimeDev fill");
        must(pd[i].f64 ? pd[i].colw[32] != 0.0 : pd[i].colw[0] == 0.0, "column twiddles: the fp64 engine's alone");
    }
    k2_lift_masks(P, pd.data());
    u64 f64_targets = 0;
    for (size_t t = 0; t < P.K; ++t) f64_targets |= (u64)(P.primes[t].f64 ? 1 : 0) << t;
    for (size_t j = 0; j < P.K; ++j)
        must(!(pd[j].k2_direct & pd[j].k2_lift) && !((pd[j].k2_direct | pd[j].k2_lift) & ~f64_targets), "lift masks: one class per fp64-engine target");
    const std::vector<FloorConst> fc = floor_const_table(P);
    must(fc.size() == P.K * P.K, "floor table size");
    for (size_t s = 0; s < P.K; ++s)
        for (size_t i = 0; i < P.K; ++i) {
            const FloorConst &f = fc[s * P.K + i];
            const u64 qs = P.primes[s].q, qi = P.primes[i].q;
            if (s == i) must(f.inv == 0 && f.inv_shoup == 0 && f.half_mod == 0 && f.src_mod == 0, "floor table diagonal");
            else must((u64)(((u128)f.inv * (qs % qi)) % qi) == 1 && f.src_mod == qs % qi && f.half_mod == (qs >> 1) % qi && f.inv_d == (double)f.inv, "floor constants");
        }
    for (int L : {1, (int)P.Ltop}) {
        const CrtTablesHost c = crt_tables_host(P, L);
        must(c.words == L + 2 && c.h.size() == c.o_inv + (size_t)L && c.Qd > 0, "CRT block layout");
        for (int i = 0; i < L; ++i) {
            const u64 qi = P.primes[i].q;
            must(mw_mod(c.h.data(), c.words, qi) == 0, "Q is a multiple of every prime");
            const u64 pm = mw_mod(c.h.data() + c.o_punct + (size_t)i * c.words, c.words, qi);
            must((u64)(((u128)pm * c.h[c.o_inv + i]) % qi) == 1, "the punctured product's inverse");
        }
        must(((c.h[c.o_half] << 1) | (c.h[0] & 1)) == c.h[0], "floor(Q / 2), low word");
    }
}

static void walk_lists(int L, size_t S, size_t N)
{
    for (u64 n : kBatches) {
        const Indexer3 shapes[] = {
            {0, 0, 1, 1, 1, 0, 1, 0},                 // pairwise
            {0, 0, ~(u64)0, 3, 0, 1, 0, 1},           // an outer product: gs >= n
            {5, 7, n ? n : 1, 2, 0, 1, 0, 1},         // gs == n
            {0, 0, 80, 8, 10, 1, 8, 1},               // groups of a matrix product
            {2, 3, 6, 4, 1, 5, 3, 1},                 // b1 does not divide gs
            {0, 0, 3, 2, 1, 1, 1, 1},                 // gs does not divide 2^32 or 2^63
        };
        for (const Indexer3 &ix : shapes) {
            const BehzLists g = behz_lists(ix, n, L, S, N);
            must(g.na == g.G * g.I && g.n_cts == g.na + g.G * g.J, "the lists' sizes");
            must(g.per_res == (3 * (size_t)L + 3 * S) * N && g.per_op == (7 * (size_t)L + 7 * S) * N, "words per result");
            if (g.may_list) must(g.n_cts <= n && (g.G == 1 || n % ix.gs == 0), "lists: whole groups, no more operands than results");
            if (n == 1) must(!g.may_list && g.G == 1 && g.I == 1 && g.J == 1, "one result reads two operands");
            if (n && n <= ((u64)1 << 32) && g.may_list) { // the last result's ordinals lie inside the lists
                BehzSrc s{};
                s.ix = ix; s.I = g.I; s.J = g.J; s.na = g.na;
                must(ord_a(s, n - 1) < g.na && ord_b(s, n - 1) >= g.na && ord_b(s, n - 1) < g.n_cts, "ordinals inside the lists");
            }
        }
    }
}

int main()
{
    // N = 1024 (logn1 = 0) and N = 32768 (logn1 = 5); a one-prime chain, the smallest key-switching chain and a deep one
    for (size_t N : {(size_t)1024, (size_t)32768}) {
        // ... and chains of one engine: {50, 50} the u64 engine's, {45, 44, 46} the fp64 engine's
        for (const std::vector<int> &bits : {std::vector<int>{50}, std::vector<int>{50, 50}, std::vector<int>{45, 44, 46}, std::vector<int>{60, 45, 40, 60, 45, 40, 45, 60}}) {
            std::unique_ptr<Params> pp(Params::create(kSchemeCKKS, N, bits, 0, false));
            GOOD("shape rules", walk_shapes(*pp));
            GOOD("launch geometry", walk_launches(*pp));
            GOOD("device tables", walk_tables(*pp));
        }
        std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 60}, 20, false));
        GOOD("shape rules, BFV context", walk_shapes(*pb));
        GOOD("device tables, BFV context", walk_tables(*pb));
        for (int L : {1, 2}) GOOD("BEHZ lists", walk_lists(L, pb->behz_nB(L) + 1, N));
    }
    GOOD("launch geometry, kMaxPrimes primes", walk_full_lists());
    { // the largest grid of the case table: the headline chain {60, 45 x 15, 60} at N = 32768, L = 16, 512 ciphertexts
        std::vector<int> bits(17, 45);
        bits.front() = bits.back() = 60;
        std::unique_ptr<Params> ph(Params::create(kSchemeCKKS, 32768, bits, 0, false));
        GOOD("launch geometry, headline chain", walk_launches(*ph));
    }
    if (failures) return 1;
    std::printf("shape_rules ok\n");
    return 0;
}
