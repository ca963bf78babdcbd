// ks_shape.h -- which kernel sequence one chunk of a key switch takes, and how much scratch an op of it needs: the host rule behind
// DeviceContext::key_switch_batch, he355_rotate_sum's level sums and he355_rescale's two-launch form, spelt once.  The rules read two
// things.  KsDims: the dimensions of the kernel environment the chunk runs in (KernelEnv, he355_kernels.h: ks_dims) -- a BFV context's
// batch_env(0, true) runs on the CKKS pipeline, so the environment's scheme is not the context's.  KsLimits: the context's own ring and
// chain (Params::N, Params::K) and its limits (HE355_LATENCY_MAX / he355_set_latency_max, HE355_LDS_MAX / he355_set_lds_max, HE355_CHUNK /
// he355_set_chunk).  Arenas, streams and launches stay with the device context.  Host-only on purpose (he_params.h alone, no HIP header),
// in the style of rotation_plan.h: tests/csim returns the rules to tests/test_launch_plan_cpu.py, which holds tests/launch_plan.py's
// restatement to them, and tests/shape_rules_main.cpp walks their edges under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>

#include "he_params.h"

namespace he355 {

struct KsDims {
    int scheme, logn1, K;
};
struct KsLimits {
    u64 N = 0;            // the context's ring and chain length (Params::N, Params::K)
    int K = 0;
    u64 lat_max = 0;      // largest batch that takes the latency shape once set (HE355_LATENCY_MAX; 0: never) ...
    bool lat_auto = true; // ... until then lat_limit()'s rule
    bool lds_auto = true; // lds_limit()'s rule until set_lds_max (HE355_LDS_MAX)
    u64 lds_max = 0;
    size_t chunk = 1024;  // ciphertexts per chunk (HE355_CHUNK / he355_set_chunk)
    // he355_set_latency_max / he355_set_lds_max (and the two environment variables): n batches at most; ~0: back to the rule
    void set_latency_max(u64 n) { lat_auto = n == ~(u64)0; lat_max = lat_auto ? 0 : n; }
    void set_lds_max(u64 n) { lds_auto = n == ~(u64)0; lds_max = lds_auto ? 0 : n; }
};

// layout of the scratch arena (one per stream) for one op at level L, in words (DeviceContext::scratch cuts it up)
inline size_t scratch_words_per_op(size_t N, int L)
{
    const size_t LN = (size_t)L * N;
    return 2 * LN + LN + LN + (size_t)(L + 1) * LN + 2 * LN + 2 * N + 2 * N + 2 * LN + 3 * N + 3 * LN;
}
// the one halving loop: c, halved until fits(c) says yes; 0 when not even one fits
template <class F> size_t halve_until_fit(size_t c, F &&fits)
{
    for (;; c = (c + 1) / 2) {
        if (fits(c)) return c;
        if (c == 1) return 0;
    }
}

// The fused mod-down (CKKS only); whether it pays for a batch is fuse_pays' rule.
inline bool k3_can_fuse(const KsDims &e) { return e.scheme == kSchemeCKKS && e.K >= 2; }
// where the ring-in-LDS kernels run (L <= 6: the partial products, (2L + 4) L N words per ciphertext, live in the key-switch arena behind c01 -- (L + 10) L N words)
inline bool ks_lds_supported(const KsDims &e, int L) { return e.logn1 >= 0 && e.logn1 <= 3 && L >= 1 && L <= 6 && e.K >= 2 && L <= e.K - 1; }

// The fused mod-down runs the special prime's tiles as a launch of their own, ahead of the data primes' (their epilogue needs its
// result): n1 rows x nc / 8 op-groups of blocks.  With a handful of ciphertexts at a small ring that launch is a few dozen blocks
// on 256 CUs -- as long as the data primes' launch and nearly idle -- and the unfused sequence (every prime's tiles in ONE launch,
// then the two floor kernels) is the shorter chain: fused from 128 such blocks up.
inline bool fuse_pays(const KsDims &e, u64 nc, int L)
{
    // ... or from 1536 (tile, op-group) units of the data primes' launch up: at L = 16 that launch is 16 times the special prime's, and what
    // the fused epilogue saves (the sums' trip through HBM, k_floor_rows) outweighs the idle launch ahead of it from 17 ciphertexts on at
    // N = 2^15 instead of 25 (batch 20 / 24 of the headline shape: 1.64 -> 1.45 / 1.79 -> 1.52 ms, DotProduct -9 %; profiles/r05_latency_boundary.txt)
    const u64 sp_blocks = ((u64)1 << e.logn1) * ((nc + 7) / 8);
    return sp_blocks >= 128 || sp_blocks * (u64)L >= 1536;
}
// he355_rotate_sum: the level's sum formed by k_k3 itself (KsGroups::sum_out).  The launch then has (tiles x n / 8) blocks however many
// groups the level has, so it needs enough of them to fill the chip, groups of a multiple of eight ciphertexts, the fused path for
// every chunk, and counts that leave bit 31 free.
inline bool level_sum_pays(const KsDims &e, const KsLimits &c, int L, u64 n)
{
    if (n % 8 || !k3_can_fuse(e) || !fuse_pays(e, n, L) || (u64)c.chunk < n) return false; // (a launch holds whole groups, and takes the fused path)
    return (((u64)L << e.logn1) * (n / 8)) >= 512;                                       // blocks of the data-prime launch
}
// latency shape of the key switch: batches of at most lat_limit() ciphertexts, CKKS pipeline
// digit groups per fp64-engine tile (480 tiles x 4 single-wave blocks fill the chip once at batch 1), per u64-engine tile (64 tiles, rows
// 2.5x as long), blocks per column for the targets of k_k2n / k_floor_colsn
constexpr int kLatTargets = 8;
// Digit groups per tile of the latency shape (n_split > 1 is what selects the shape).  fp64-engine
// tiles: 480 x 2 single-wave blocks are ONE round of the chip's 1024 one-wave slots, 480 x 4 were two rounds of half the work each with
// twice the start-ups and partial sums (batch 1: 0.326 -> 0.312 ms, batch 8: 0.98 -> 0.91 ms; 3 and 8 groups measured slower).
constexpr int kLatSplit = 2, kLatSplitU64 = 8;
// Where the latency shape stops paying is a matter of rows, not of ciphertexts: the throughput kernels fill the chip from about 2^17
// coefficients per residue on (profiles/r05_latency_boundary.txt: N = 2^15 crosses between 4 and 5 ciphertexts at depth 6 and 16, 2^14
// between 6 and 8, 2^13 at 12), so the default limit is 2^17 / N ciphertexts, at most 12; he355_set_latency_max replaces it.
inline u64 lat_limit(const KsLimits &c) { return c.lat_auto ? std::min<u64>(12, std::max<u64>(1, ((u64)1 << 17) / c.N)) : c.lat_max; }
// ... for a kernel environment (a BFV context runs its rotation chains in the NTT domain on the CKKS pipeline: batch_env(0, true))
inline bool latency_shape(const KsDims &e, const KsLimits &c, u64 nc) { return e.scheme == kSchemeCKKS && nc <= lat_limit(c) && c.K >= 2; }
// Ring-in-LDS shape (he355_kernels_lds.hip): N <= 8192, L <= 6, NTT-domain pipeline, batches up to lds_limit() -- two
// launches of L^2 + 2L one-polynomial workgroups per ciphertext instead of six launches through HBM.  Where the throughput shape's
// better use of the chip overtakes it was measured (profiles/r06_lds_shape.txt); he355_set_lds_max / HE355_LDS_MAX replace the rule.
// The rule: while k_lds_digits' grid, (L + 1) L blocks per ciphertext, runs in at most one and a half rounds of the chip -- 256 CUs, one
// 8-wave block each at N = 8192 (two, four, eight blocks per CU for the smaller rings): 64 ciphertexts at {60, 40, 60} (32: 61 against 78 us
// per key switch, 64: 89 against 95, 96: 131 against 113), 32 at {60, 40, 40, 60}; beyond that the HBM throughput shapes use the chip
// better (profiles/r06_lds_shape.txt; a "one inverse transform, every target" form of the kernels for larger batches was built, bit-exact,
// and lost everywhere: same file, tools/patches/r06_lds_source_major.patch).  he355_set_lds_max / HE355_LDS_MAX replace the rule.
inline u64 lds_limit(const KsDims &e, const KsLimits &c, int L)
{
    if (!c.lds_auto) return c.lds_max;
    const u64 blocks = (u64)384 << (3 - std::min(3, e.logn1));
    return std::max<u64>(1, blocks / ((u64)(L + 1) * (u64)L));
}
// (also the test of he355_rescale's two-launch form)
inline bool lds_shape(const KsDims &e, const KsLimits &c, int L, u64 nc) { return e.scheme == kSchemeCKKS && ks_lds_supported(e, L) && nc <= lds_limit(e, c, L); }

// What a key switch switches.  key_switch_batch alone turns it into k_k1's flags, K3Fuse's operand fields and LdsKsOperands.
enum class KsKind {
    Product, // a * b of two size-2 ciphertexts: a, b [.][2][L][N], result r takes a[idx_a(ix, r)], b[idx_b(ix, r)] (he355_multiply_relin)
    Size3,   // a [n][3][L][N]: c2 switched, added into (c0, c1) (he355_relinearize)
    Galois,  // a [n][2][L][N] under element elt (table: its NTT-domain permutation or coefficient-form gather), out = addend + galois(a)
    Grouped, // a [.][2][L][N] in groups of groups.group_size ciphertexts, per-group elements and keys (he355_rotate_sum, rotate_each)
};
enum class KsShape { Lds, Latency, Fused, Unfused, BfvCoeff };
// The shape of one chunk's key switch: the whole rule.  The first row that holds:
//   BfvCoeff | e.scheme is BFV: coefficient-form ciphertexts of a BFV context (the BFV kernels; no he355_path_stats counter)
//   Lds      | not grouped, out_apart, lds_shape(e, c, L, nc): CKKS / NTT-domain pipeline, ks_lds_supported(e, L), nc <= lds_limit(e, c, L)
//   Latency  | not grouped, latency_shape(e, c, nc)
//   Fused    | k3_can_fuse(e), fuse_pays(e, nc, L)  (and c01 a slab [nc][2][L][N] of its own: key_switch_batch always lays it out so)
//   Unfused  | otherwise
// out_apart: `out` shares no word with a product's operands or a size-3 input (a rotation may add into `out`: always apart).  k_k3 forms
// c0, c1 itself (K3Fuse operands, k_k1 does not write them) exactly when the shape is Fused and out_apart.
inline KsShape ks_shape(const KsDims &e, const KsLimits &c, int L, u64 nc, KsKind kind, bool out_apart)
{
    if (e.scheme != kSchemeCKKS) return KsShape::BfvCoeff;
    if (kind != KsKind::Grouped && out_apart && lds_shape(e, c, L, nc)) return KsShape::Lds;
    if (kind != KsKind::Grouped && latency_shape(e, c, nc)) return KsShape::Latency;
    return k3_can_fuse(e) && fuse_pays(e, nc, L) ? KsShape::Fused : KsShape::Unfused;
}

} // namespace he355
