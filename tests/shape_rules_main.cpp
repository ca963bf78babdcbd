// shape_rules_main.cpp -- TEST-ONLY, stand-alone.  Walks the device context's host rules -- csrc/ks_shape.h, csrc/device_tables.h and
// csrc/behz_lists.h -- at their edges: batches of 0, 1, 2^32 and 2^63, L = 1 and L_top, logn1 = 0 and 5 (N = 1024 and 32768), a one-prime
// chain (K = 1), each limit set to 0 (the shape is never taken), to 2^64 - 1 (the rule applies again) and to 2^64 - 2, indexers with gs >= n and
// with gs that does not divide n -- compiled with -fsanitize=address,undefined (tests/test_launch_plan_cpu.py).  The rules shift by logn1,
// multiply batch sizes the caller chose and index tables by prime: none of it may overflow a signed type, shift out of range, divide by zero or
// reach outside a vector (unsigned wrap at an absurd batch is the product's behaviour and stays).  Where a value can be checked in a line it
// is: the tables' inverses invert, the masks name fp64-engine targets only, the lists of a batch hold every operand a result reads.
// Prints "shape_rules ok" and exits 0, or names the first case that went the other way.
#include <cstdio>
#include <memory>
#include <vector>

#include "../reference-seal-backend_amd/csrc/behz_lists.h"
#include "../reference-seal-backend_amd/csrc/device_tables.h"
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
        for (const std::vector<int> &bits : {std::vector<int>{50}, std::vector<int>{50, 50}, std::vector<int>{60, 45, 40, 60, 45, 40, 45, 60}}) {
            std::unique_ptr<Params> pp(Params::create(kSchemeCKKS, N, bits, 0, false));
            GOOD("shape rules", walk_shapes(*pp));
            GOOD("device tables", walk_tables(*pp));
        }
        std::unique_ptr<Params> pb(Params::create(kSchemeBFV, N, {60, 40, 60}, 20, false));
        GOOD("shape rules, BFV context", walk_shapes(*pb));
        GOOD("device tables, BFV context", walk_tables(*pb));
        for (int L : {1, 2}) GOOD("BEHZ lists", walk_lists(L, pb->behz_nB(L) + 1, N));
    }
    if (failures) return 1;
    std::printf("shape_rules ok\n");
    return 0;
}
