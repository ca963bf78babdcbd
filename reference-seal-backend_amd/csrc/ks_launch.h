// ks_launch.h -- the launch geometry of the key-switch kernels, spelt once: which kernels of a chunk's sequence (ks_shape.h) run as one
// launch for both engines or as one per engine, with which grid, and what each launch's argument block says about its share of the work
// (the engine's primes, op-groups per block, waves, target split).  The launchers of he355_kernels_ks.hip (launch_k1, launch_k2,
// launch_floor_cols, launch_floor_rows), he355_kernels_k3.hip (launch_k3, launch_k3_combine) and he355_kernels.hip
// (launch_rows_inv_select) call these functions, fill the kernels' argument blocks
// from the operands and the plan, and launch; nothing here reserves, launches or counts.  The rules read KsLaunchDims, what a launcher
// reads of its KernelEnv (he355_kernels.h: ks_launch_dims).  Host-only, like ks_shape.h (no HIP header): tests/csim returns the plans to
// tests/test_launch_plan_cpu.py, which holds tests/launch_plan.py's restatement to them, and tests/shape_rules_main.cpp walks their edges
// under the sanitizers.
#pragma once
#include <algorithm>
#include <stdexcept>

#include "device_types.h"
#include "ks_shape.h"

namespace he355 {

// The block the row kernels' grids assume: kWaves waves of 64 lanes, one row job per wave (kernel_common.inc takes both from here).
constexpr int kBlock = 256;
constexpr int kWaves = 4;
// The two engines' launches of a stage as one kernel (k_k1_dual, k_k2n_dual, k_k3_dual, k_floor_rows_dual) in the latency shape, and
// for small grids of the throughput shape: up to this many blocks for both engines together (profiles/r04_dual_engine_latency.txt)
// (round 5: per kernel.  k_k3's shared launch pays up to a few thousand blocks since the fold form of the u64 engine brought its blocks
// close to the fp64 engine's in length; the others -- whose dual kernels are the latency shape's, behind a function boundary -- keep
// the 1024 they were swept at.  profiles/r05_dual_threshold_sweep.txt)
constexpr unsigned kDualMaxBlocksK3 = 4096, kDualMaxBlocks = 1024;

struct KsLaunchDims {
    int scheme, logn1, K;
    const unsigned char *prime_f64; // [K] 1: the fp64 engine owns prime i
    const u64 *prime_q;             // [K] the moduli
};
inline unsigned blocks_for(u64 jobs, u64 per_block) { return (unsigned)((jobs + per_block - 1) / per_block); }

// ---- engine helpers ---------------------------------------------------------------------------------------------------------------
struct IndexList {
    unsigned char at[kMaxPrimes];
    int n = 0;
};
// The engine partition: the indices i of [0, n) whose prime prime_of(i) the fp64 engine owns (f64) or does not own, in order;
// prime_of(i) < 0 leaves i out of the range.
template <class PrimeOf> IndexList engine_list(const unsigned char *prime_f64, bool f64, int n, PrimeOf &&prime_of)
{
    IndexList l;
    for (int i = 0; i < n; ++i) {
        const int p = prime_of(i);
        if (p >= 0 && (prime_f64[p] != 0) == f64) l.at[l.n++] = (unsigned char)i;
    }
    return l;
}
// a list into the fixed array and count of a kernel's argument block
template <size_t N> void copy_list(unsigned char (&dst)[N], int &n, const IndexList &l)
{
    static_assert(N >= sizeof(l.at), "an argument block's list holds every prime");
    n = l.n;
    std::copy(l.at, l.at + l.n, dst);
}
// bit t: the fp64 engine owns target prime t (k_k2n, k_floor_colsn)
inline u64 f64_mask(const KsLaunchDims &e)
{
    u64 m = 0;
    for (int t = 0; t < e.K; ++t) m |= (u64)(e.prime_f64[t] != 0) << t;
    return m;
}

// ---- K1 ---------------------------------------------------------------------------------------------------------------------------
struct K1Geometry {
    IndexList i_list[2]; // [0]: fp64-engine residues, [1]: u64-engine residues
    bool dual;           // k_k1_dual: grid dual_grid[0] + dual_grid[1], the first dual_grid[0] blocks the fp64 engine's
    unsigned dual_grid[2];
    unsigned grid[2];    // k_k1 proper -- the throughput shape -- maps a block onto one (residue, row) tile and four consecutive ops; 0: no launch
};
// c2_only: the ct x ct multiply that leaves c0, c1 to the fused k_k3 (K1Operands::no_c01) has no dual kernel
inline K1Geometry k1_geometry(const KsLaunchDims &e, int L, u64 n_ops, bool c2_only)
{
    K1Geometry G;
    for (int pass = 0; pass < 2; ++pass) {
        G.i_list[pass] = engine_list(e.prime_f64, pass == 0, L, [](int i) { return i; });
        const int n_i = G.i_list[pass].n;
        G.dual_grid[pass] = n_i ? blocks_for((n_ops * n_i) << e.logn1, kWaves) : 0;
        G.grid[pass] = n_i ? (unsigned)((((u64)n_i) << e.logn1) * ((n_ops + kWaves - 1) / kWaves)) : 0;
    }
    const unsigned *gp = G.dual_grid;
    // latency shape / small grids: one launch for both engines
    G.dual = gp[0] && gp[1] && (n_ops <= 8 || gp[0] + gp[1] <= kDualMaxBlocks) && !c2_only;
    return G;
}

// ---- K2 ---------------------------------------------------------------------------------------------------------------------------
// Small grids: the targets of a (digit, column block) dealt to 2 or 4 blocks (blockIdx.y, as the latency shape does) when
// that fills the rounds of blocks better -- 512 blocks run at a time (two per CU); a block pays the digit's inverse column
// pass once and a forward column pass + stores per target.  64 BFV ciphertexts at L = 3: 768 blocks = 1.5 rounds of all four
// targets, or 3 full rounds of two targets each.  Only taken for a modelled gain of 5 % or more (the headline's 61440 blocks
// stay whole).
inline int k2_target_split(const KsLaunchDims &e, int L, unsigned gw, int tsplit)
{
    if (tsplit > 1) return tsplit;
    int ts = 1;
    const int n_tgt = L + 1 - (e.scheme == kSchemeCKKS ? 1 : 0);
    auto cost = [&](int c) { return (double)(((u64)gw * c + 511) / 512) * (1.0 + 1.2 * ((n_tgt + c - 1) / c)); };
    const double c1 = cost(1);
    double best = c1;
    for (int c = 2; c <= 4; c <<= 1)
        if (cost(c) < best * 0.95 && cost(c) < c1 * 0.95) { best = cost(c); ts = c; }
    return ts;
}
struct K2Geometry {
    IndexList dig_list[2]; // digits below 2^52, then the 60-bit ones: one instantiation each
    unsigned gx[2];        // blocks of each kind (gridDim.x); 0: no such digit
    bool dual;             // k_k2n_dual: grid (gx[0] + gx[1], ts[0]), both kinds with ts[0]
    int ts[2];             // target split (gridDim.y) of each kind's own launch
};
inline K2Geometry k2_geometry(const KsLaunchDims &e, int L, u64 n_ops, int tsplit)
{
    K2Geometry G;
    for (int wide = 0; wide < 2; ++wide) {
        IndexList &l = G.dig_list[wide];
        for (int j = 0; j < L; ++j)
            if ((e.prime_q[j] >> 52 != 0) == (wide != 0)) l.at[l.n++] = (unsigned char)j;
        G.gx[wide] = (unsigned)(n_ops * l.n * 4);
    }
    G.dual = false;
    if (G.gx[0] && G.gx[1]) { // latency shape or a small grid: both digit kinds in one launch (k_k2n_dual)
        const int ts = k2_target_split(e, L, G.gx[0] + G.gx[1], tsplit);
        if (tsplit > 1 || (G.gx[0] + G.gx[1]) * (unsigned)ts <= kDualMaxBlocks) {
            G.dual = true;
            G.ts[0] = G.ts[1] = ts;
            return G;
        }
    }
    for (int wide = 0; wide < 2; ++wide) G.ts[wide] = G.gx[wide] ? k2_target_split(e, L, G.gx[wide], tsplit) : 1;
    return G;
}

// ---- K3 ---------------------------------------------------------------------------------------------------------------------------
// `part`: all tiles, only the special prime's, or only the data primes'
enum K3Part { K3_ALL = 0, K3_SPECIAL_ONLY = 1, K3_DATA_ONLY = 2 };
struct K3Request {
    int L;
    u64 n_ops;
    K3Part part = K3_ALL;
    bool fuse = false;        // the mod-down in the epilogue, data primes tt_lo <= tt < tt_hi (K3Fuse)
    int tt_lo = 0, tt_hi = 0;
    bool rescale = false;     // ... with the second floor step (K3Fuse::cols2)
    int n_split = 1, n_split_u64 = 0; // digit groups per fp64-engine / u64-engine tile; > 1 selects the latency shape
    bool grouped = false;     // KsGroups: group_size consecutive ops per group, the launch's first op is op g_op_offset of the call
    u32 group_size = 0;
    bool sum_out = false;     // KsGroups::sum_out
    u64 g_op_offset = 0;
};
struct K3Grid {
    u64 n_og;         // op-groups of w ops
    u32 og_per_block; // consecutive op-groups one block handles on its tile
    unsigned g;       // blocks
};
// Op-groups per block: more of them amortise the block's start-up (twiddle staging, ~4 us) over more work, fewer of them give the
// dispatcher more blocks to fill the 256 CUs with.  What counts for small grids is the number of ROUNDS of blocks: 64 tiles x 8
// op-groups (BFV, 64 ciphertexts, L = 3) are two rounds of 256 one-group blocks or ONE round of two-group blocks, the same work
// with half the start-ups (configs[4]: 65.3 -> 63.4 ms).  So: the candidate sizes from the shape's maximum down, each priced as
// rounds x (groups x work per group + start-up), ties to the larger.  (Maximum for the 8-wave shape: 4 once a tile has 128
// op-groups -- chunks of 1024 ciphertexts: 50.3 vs 50.9 ms per step with 2 -- and 2 below that, where 4 measured slower;
// profiles/r03_chunk_sweep.txt.)
inline K3Grid k3_size_grid(u64 tiles, u64 n_ops, int w, bool f64, int L)
{
    K3Grid r;
    r.n_og = (n_ops + w - 1) / w;
    const u32 og_max = w == 8 ? (r.n_og >= 128 ? 4 : 2) : 4;
    r.og_per_block = og_max;
    const double work = (f64 ? 7.0 : 14.0) * (L + 2) * (w == 4 ? 0.5 : 1.0), startup = 4.0; // us per op-group (one row step per digit + epilogue), per block
    double best = 0;
    for (u32 c = og_max; c >= 1; c >>= 1) {
        const u64 blocks = tiles * ((r.n_og + c - 1) / c);
        const double cost = (double)((blocks + 255) / 256) * (c * work + startup);
        if (c == og_max || cost < best * 0.999) { best = cost; r.og_per_block = c; }
    }
    const u64 n_ogb = (r.n_og + r.og_per_block - 1) / r.og_per_block;
    r.g = (unsigned)(((tiles + 7) / 8) * 8 * n_ogb);
    return r;
}
struct K3Pass {          // one engine's tiles
    bool f64;
    IndexList tt_list;   // the key primes tt (L: the special prime) of the engine's tiles
    unsigned char q_slot[kMaxPrimes]; // tt_list[k] -> its index among the u64-engine primes of the key chain
    int n_split;         // digit groups per tile (gridDim.y of the engine's own launch)
    int waves;           // 1: latency shape, one (tile, op, digit group) per block; 8; 4: u64-engine tiles of a small grid
    u32 og_per_block, og_stride;
    unsigned g;          // blocks (gridDim.x)
};
enum class K3Form {
    Dual,     // k_k3_dual: both engines' single-wave blocks, grid (g0 + g1, the larger n_split), 64 threads
    Dual8,    // k_k3_dual8<..., u64 waves>: grid g0 + g1, 512 threads
    Separate, // k_k3 per engine: grid (g, n_split), 64 x waves threads
};
struct K3Geometry {
    K3Pass pend[2]; // fp64 engine first
    int n_pend = 0;
    int n_q = 0;    // u64-engine primes in the key chain
    bool level_sum = false;
    K3Form form = K3Form::Separate;
};
inline K3Geometry k3_geometry(const KsLaunchDims &e, const K3Request &r)
{
    const int L = r.L;
    const int n_split_u64 = r.n_split_u64 <= 0 ? r.n_split : r.n_split_u64;
    if (r.n_split > 1 && r.fuse) throw std::runtime_error("digit-split K3: unfused launches with a partial-sum buffer only");
    K3Geometry G;
    if (!r.n_ops) return G;
    if (r.fuse && r.rescale && r.tt_hi > L - 1) throw std::runtime_error("fused rescale: only primes below the one divided out");
    for (int t = 0; t < e.K; ++t) G.n_q += e.prime_f64[t] == 0;
    G.level_sum = r.grouped && r.sum_out && r.fuse; // (the special prime's launch ahead of it writes no ciphertext rows)
    for (int pass = 0; pass < 2; ++pass) { // pass 0: fp64-engine primes, pass 1: u64-engine primes
        K3Pass P;
        P.f64 = pass == 0;
        P.tt_list = engine_list(e.prime_f64, P.f64, L + 1, [&](int tt) {
            if ((r.part == K3_SPECIAL_ONLY && tt != L) || (r.part == K3_DATA_ONLY && tt == L)) return -1;
            if (r.fuse && (tt < r.tt_lo || tt >= r.tt_hi)) return -1;
            return tt == L ? e.K - 1 : tt;
        });
        if (!P.tt_list.n) continue;
        for (int k = 0; k < P.tt_list.n; ++k) {
            const int tt = P.tt_list.at[k], t = tt == L ? e.K - 1 : tt;
            int slot = 0;
            for (int u = 0; u < t; ++u) slot += e.prime_f64[u] == 0;
            P.q_slot[k] = (unsigned char)slot;
        }
        P.n_split = r.n_split > 1 ? (pass == 0 ? r.n_split : n_split_u64) : 1;
        P.waves = P.n_split > 1 ? 1 : 8; // latency shape: one wave per block, one (tile, op, digit group) each; else the 8-wave shape
        const u64 tiles = (u64)P.tt_list.n << e.logn1;
        // enough blocks to keep every CU busy for several rounds, few enough that start-up costs are amortised
        K3Grid sg = k3_size_grid(tiles, r.n_ops, P.waves, P.f64, L);
        if (G.level_sum) {
            // one block per (tile, eight ciphertexts), walking this launch's groups in turn (see KsGroups::sum_out)
            const u64 gs8 = r.group_size / 8;
            if (P.waves != 8 || r.group_size % 8 || r.n_ops % r.group_size || r.g_op_offset % r.group_size)
                throw std::runtime_error("level sum in k_k3: fused 8-wave launches over whole groups of a multiple of eight ciphertexts");
            sg.og_per_block = (u32)(sg.n_og / gs8);
            sg.g = (unsigned)(((tiles + 7) / 8) * 8 * gs8);
        }
        // u64-engine tiles of a small grid (at most half the CUs busy with 8-wave blocks): FOUR waves per block -- one per SIMD, each at
        // the full issue rate instead of half of it, and twice the blocks; the serial digit loop of a tile is what such a launch lasts
        if (pass == 1 && P.waves == 8 && sg.g <= 128 && !G.level_sum) {
            const K3Grid s4 = k3_size_grid(tiles, r.n_ops, 4, P.f64, L);
            // (a CU holds ONE block of either shape -- the LDS arrays -- so the four-wave blocks must still fit one round together with the
            // fp64-engine blocks they may share the launch with)
            if (s4.g + (G.n_pend ? G.pend[0].g : 0) <= 256) { P.waves = 4; sg = s4; }
        }
        P.og_per_block = sg.og_per_block;
        P.og_stride = G.level_sum ? (u32)(r.group_size / 8) : 1u;
        P.g = sg.g;
        G.pend[G.n_pend++] = P;
    }
    if (G.n_pend == 2 && G.pend[0].waves == 1) G.form = K3Form::Dual; // latency shape
    // throughput shape, small grids (up to two blocks per CU for both engines together): both engines in one launch
    else if (G.n_pend == 2 && G.pend[0].waves == 8 && G.pend[0].g + G.pend[1].g <= kDualMaxBlocksK3) G.form = K3Form::Dual8;
    return G;
}
inline unsigned k3_combine_grid(const KsLaunchDims &e, int L, u64 n_ops) { return blocks_for((n_ops * 2 * (u64)(L + 1)) << e.logn1, kWaves); }

// ---- the floor step ---------------------------------------------------------------------------------------------------------------
struct FloorColsGrid {
    unsigned x, y; // y: the target split
};
inline FloorColsGrid floor_cols_grid(u64 n_polys, int tsplit) { return FloorColsGrid{(unsigned)(n_polys * 4), (unsigned)(tsplit > 1 ? tsplit : 1)}; }
struct FloorRowsGeometry {
    u32 jobs_per_block;
    // the (engine, tail) passes -- [0] fp64 engine, [1] its tail prime, [2] u64 engine, [3] its tail prime: the tail prime gets a launch of
    // its own (k_floor_rows<engine, tail>); g 0: no launch
    IndexList i_list[4];
    unsigned g[4];
    bool dual; // no tail prime; latency shape or small grids: passes 0 and 2 in one launch (k_floor_rows_dual, the first g[0] blocks the fp64 engine's)
};
inline FloorRowsGeometry floor_rows_geometry(const KsLaunchDims &e, u64 n_ops, int n_tgt, int n_src, int tail_prime)
{
    FloorRowsGeometry G;
    const u64 n_jobs = n_ops * n_src;
    // per block: up to 8 jobs per wave, fewer when that would leave CUs without blocks
    u32 jpb = 8 * kWaves;
    while (jpb > (u32)kWaves && (((u64)n_tgt << e.logn1) * ((n_jobs + jpb - 1) / jpb) < 256u * 8 || jpb / 2 >= n_jobs)) jpb >>= 1;
    G.jobs_per_block = jpb;
    for (int pass = 0; pass < 4; ++pass) {
        const bool tail = pass & 1;
        G.i_list[pass] = engine_list(e.prime_f64, pass < 2, n_tgt, [&](int i) { return (i == tail_prime) == tail ? i : -1; });
        G.g[pass] = (unsigned)((((u64)G.i_list[pass].n) << e.logn1) * ((n_jobs + jpb - 1) / jpb));
    }
    G.dual = tail_prime < 0 && G.g[0] && G.g[2] && (n_ops <= 8 || G.g[0] + G.g[2] <= kDualMaxBlocks);
    return G;
}
inline unsigned rows_inv_select_grid(const KsLaunchDims &e, u64 n_polys) { return blocks_for(n_polys << e.logn1, kWaves); }

} // namespace he355
