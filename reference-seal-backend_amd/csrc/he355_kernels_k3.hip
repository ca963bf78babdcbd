// he355_kernels_k3.hip -- the key product of the hybrid key switch (DESIGN.md "Key-switch pipeline"): per (op, key prime, row) the sum
// over the digits of NTT(digit) * key, with the mod-down (and the rescale) finished in its epilogue where the caller fuses them.
//
//   k_k3                       the template kernel (body: k3_body.inc), one instantiation per (engine, waves, FUSE, TENSOR, GROUPED)
//   k_k3_dual, k_k3_dual8      both engines' tiles of one stage in one launch (the same body behind a function boundary)
//   k_k3_combine               the sums of a digit-split launch (latency shape) added up, special prime through its inverse row pass
//
// What comes before and after it -- K1, K2, the floor step -- is he355_kernels_ks.hip; grids and engine splits: ks_launch.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <type_traits>

#include "he355_kernels.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_k3.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// =======================================================================================================
// K3: per (op, key prime tt, row): sum over digits j of NTT_tt(digit j) * key_j[k][tt]
// =======================================================================================================
struct K3Args {
    const u64 *d, *c2n, *key;
    const u64 *cols;   // FUSE: mod-down corrections after the forward column pass [n_ops*2][L][N] (raw of prime tt)
    u64 *c01; u64 c01_item_stride; // FUSE: polys that receive (T - NTT(cols)) * P^-1
    const FloorConst *fc;          // FUSE: floor constants [K][K]
    const u64 *cols2; u64 *out2;   // FUSE + rescale: second correction slab [n_ops*2][L-1][N] and the final output [n_ops][2][L-1][N]
    int c1_mode; const u64 *c1_src; // FUSE, rotations: the floor step's addend of polynomial 1 is zero (1) / a row of c1_src (2) instead of a c01 row (0)
    const u64 *gsrc; const uint32_t *gperm; u64 gsrc_op_offset; // c1_mode 4: the rotation's input, gathered here (K3Fuse::gsrc)
    const u64 *ta, *tb; Indexer tix; u64 t_op_offset; // FUSE, ct x ct multiply: the floor step's addend is a0 b0 / a0 b1 + a1 b0 of these operands (K3Fuse::ta); ta null: read from c01
    KsGroups groups; u64 g_op_offset; u64 keyq_offset; // GROUPED: op (g_op_offset + op) takes its key from groups.key[group]; its quotients follow at keyq_offset
    const u64 *keyq;   // Shoup quotients of the key residues under the u64-engine primes: [L_top][2][n_q][N]
    int n_q;           // u64-engine primes in the key chain
    unsigned char q_slot[64]; // tt_list[k] -> its index among them
    u64 *t, *tp, *tpr; // sums of the data primes; of the special prime (unused: its rows leave through tpr, inverse row pass done)
    u64 n_ops;
    int L, K, logn1, ckks;
    int n_tt;
    u32 og_per_block; // consecutive op-groups one block handles on its tile
    u32 og_stride;    // 1; level-sum launches (KsGroups::sum_out): the block's op-groups are n_ogb apart -- the same eight ciphertexts of every group
    // latency shape (few ops): the digits of a tile are cut into n_split groups, one block each (blockIdx.y); group g writes its canonical
    // partial sums to part[g][op * 2 + k][L + 1][N] and k_k3_combine adds them up (and runs the special prime's inverse row pass)
    int n_split;
    u64 *part;
    unsigned char tt_list[64];
};

// Digit rows reach the wave through an LDS landing buffer filled by LDS-DMA one step ahead.
// FUSE: the mod-down of the key switch is finished here instead of in k_floor_rows: the tile's sums never leave the
// registers — the wave transforms the matching rows of the special-prime correction (forward row pass, same tile twiddles)
// and writes (T - NTT(delta)) * P^-1 + c01 straight into c01.  Needs the special prime's sums first: the caller launches the
// special-prime tiles, the inverse transform and k_floor_colsn before the data-prime tiles.
// TENSOR: the launch belongs to a ct x ct multiply whose c0, c1 this kernel computes from the operand rows (K3Args::ta); an
// instantiation of its own, so that the other users of the fused kernel keep their register allocation.  TENSOR without FUSE is the
// rescale's divided-out prime (K3Fuse::raw_tail): the same sums and digit loop, then the inverse row pass instead of the floor step.
// WAVES: 8 (throughput shape: one block per CU, two waves per SIMD, each wave on its own op; LDS: 8 x 8.5 KiB exchange + 8 x 8 KiB
// DMA landing + the tile's twiddles) or 1 (latency shape: one wave per block, the digits of a tile dealt to n_split blocks).
// GROUPED: every group of ops has its own key (he355_rotate_sum: all nodes of a trie level in one launch); ops of a group are consecutive,
// so the waves of a block still share their key rows through L1 / L2 for a group's worth of ops.  Instantiations of its own.
template <class Ar, int WAVES, bool FUSE = false, bool TENSOR = false, bool GROUPED = false>
__global__ void __launch_bounds__(WAVES * 64) k_k3(K3Args A, const PrimeDev *primes)
{
#define K3_BID_X blockIdx.x
#define K3_BID_Y blockIdx.y
#define K3_LDS_DECL                                                                                                            \
    __shared__ u64 lds[kWaves][kLdsRow];                                                                                       \
    __shared__ __attribute__((aligned(16))) u64 stage[kWaves][kRowN];                                                          \
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kF64 ? kRowTw * 8 : kRowTw * 16];
#include "k3_body.inc"
#undef K3_BID_X
#undef K3_BID_Y
#undef K3_LDS_DECL
}
// Both engines' tiles of one stage in ONE launch: the fp64-engine blocks (0 .. n_f - 1) and the u64-engine blocks side by side, on one
// set of LDS arrays.  Two uses.  Latency shape (k_k3_dual, single-wave blocks; blockIdx.y = digit group, each engine with its own
// count, surplus blocks leave at once): a batch-1 key switch is a chain of launches of 5-12 us each, bound by launch and
// dependent-chain latency, and one launch instead of two per stage takes the shorter engine's time out of the chain.  Small grids of
// the throughput shape (k_k3_dual8: tens of ciphertexts at N = 8192 are 30-130 blocks per engine on 256 CUs): the two launches
// would run one after the other on a mostly idle chip.  (The same body text as k_k3, behind a function boundary here -- which is
// why the large grids, the headline's among them, keep the template kernels.)
// (ARGS: `const K3Args &` for the single-wave instantiations, `const K3Args` for the 8-wave ones -- whichever lets the compiler keep the
// argument struct in the kernarg segment instead of copying it to scratch: 0 vs 416 B and 68-244 vs 880-960 B per lane, tools/kres.py)
template <class Ar, int WAVES, bool FUSE, bool TENSOR, bool GROUPED, class ARGS>
__device__ __forceinline__ void k3_body_fn(ARGS A, const PrimeDev *primes, const unsigned bid_x, const unsigned bid_y, u64 (*lds)[kLdsRow],
                                           u64 (*stage)[kRowN], unsigned char *twl_raw)
{
#define K3_BID_X bid_x
#define K3_BID_Y bid_y
#define K3_LDS_DECL
#include "k3_body.inc"
#undef K3_BID_X
#undef K3_BID_Y
#undef K3_LDS_DECL
}
// the body's early-exit test (k3_body.inc: `if (tile >= total_tiles) return;`) for a block of WAVES waves
template <int WAVES> __device__ __forceinline__ bool k3_block_has_tile(const K3Args &A, unsigned bid_x)
{
    const u64 n_og = (A.n_ops + WAVES - 1) / WAVES;
    const u64 n_ogb = (n_og + A.og_per_block - 1) / A.og_per_block;
    const u64 total_tiles = (u64)A.n_tt << A.logn1;
    const u64 s = bid_x >> 3, xcd = bid_x & 7;
    return (s / n_ogb) * 8 + xcd < total_tiles;
}
__global__ void __launch_bounds__(64) k_k3_dual(K3Args AF, K3Args AU, unsigned n_u, const PrimeDev *primes)
{
    __shared__ u64 lds[1][kLdsRow];
    __shared__ __attribute__((aligned(16))) u64 stage[1][kRowN];
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kRowTw * 16];
    if (blockIdx.x < n_u) { // the u64-engine blocks first: the longer ones (see k_k3_dual8)
        if ((int)blockIdx.y < (AU.n_split > 1 ? AU.n_split : 1))
            k3_body_fn<ArU64, 1, false, false, false, const K3Args &>(AU, primes, blockIdx.x, blockIdx.y, lds, stage, twl_raw);
    } else {
        if ((int)blockIdx.y < (AF.n_split > 1 ? AF.n_split : 1))
            k3_body_fn<ArF64, 1, false, false, false, const K3Args &>(AF, primes, blockIdx.x - n_u, blockIdx.y, lds, stage, twl_raw);
    }
}
// (the u64-engine blocks come FIRST: they run 2.5 times as long as an fp64-engine block, and dispatched last they would be the launch's tail;
// UW = 4: the u64-engine blocks work with their first four waves, one per SIMD -- see launch_k3)
template <bool FUSE, bool TENSOR, bool GROUPED, int UW = 8>
__global__ void __launch_bounds__(512) k_k3_dual8(K3Args AF, K3Args AU, unsigned n_u, const PrimeDev *primes)
{
    __shared__ u64 lds[8][kLdsRow];
    __shared__ __attribute__((aligned(16))) u64 stage[8][kRowN];
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kRowTw * 16];
    if (blockIdx.x < n_u) {
        if (UW == 4 && threadIdx.x >= 256) {
            // waves 4-7 of a four-wave block do no work, but every wave of the block meets the body's one workgroup barrier (the
            // twiddle staging) -- or none does, when the block has no tile
            if (k3_block_has_tile<4>(AU, blockIdx.x)) __syncthreads();
            return;
        }
        k3_body_fn<ArU64, UW, FUSE, TENSOR, GROUPED, const K3Args>(AU, primes, blockIdx.x, 0, lds, stage, twl_raw);
    } else {
        k3_body_fn<ArF64, 8, FUSE, TENSOR, GROUPED, const K3Args>(AF, primes, blockIdx.x - n_u, 0, lds, stage, twl_raw);
    }
}

// The sums of a digit-split k_k3 launch: part [n_split][n_ops * 2][L + 1][N] canonical -> t (data primes, canonical NTT form) and tpr
// (special prime, after the inverse row pass), exactly what the unsplit launch leaves.  One wave per (op, k, tt, row).
struct K3CombineArgs {
    const u64 *part;
    u64 *t, *tpr;
    u64 n_ops;
    int n_split, n_split_u64, L, K, logn1, ckks; // digit groups of the fp64-engine / u64-engine tiles
};
__global__ void __launch_bounds__(kBlock) k_k3_combine(K3CombineArgs A, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    const u64 total = A.n_ops * 2 * (u64)(A.L + 1) * n1;
    u64 job = (u64)blockIdx.x * kWaves + wave;
    const bool valid = job < total;
    if (!valid) job = total - 1;
    const u32 a_row = (u32)(job & (n1 - 1));
    const u64 pt = job >> A.logn1;
    const int tt = (int)(pt % (A.L + 1));
    const u64 ok = pt / (A.L + 1); // op * 2 + k
    const int t = tt == A.L ? A.K - 1 : tt;
    const PrimeDev &P = primes[t];
    const u64 rowoff = (u64)a_row << kRowLog, q = P.q;
    u64 v[kRowE];
    load_rowC(A.part + (ok * (A.L + 1) + tt) * N + rowoff, lane, v);
    const int groups = P.f64 ? A.n_split : A.n_split_u64;
    for (int g = 1; g < groups; ++g) {
        u64 w[kRowE];
        load_rowC(A.part + (((u64)g * A.n_ops * 2 + ok) * (A.L + 1) + tt) * N + rowoff, lane, w);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = addmod(v[r], w[r], q);
    }
    const bool inv_here = tt == A.L || !A.ckks;
    if (!inv_here) {
        if (valid) store_rowC(A.t + (ok * A.L + tt) * N + rowoff, lane, v);
        return;
    }
    const bool last = A.logn1 == 0;
    u64 *dst = tt < A.L ? A.t + (ok * A.L + tt) * N + rowoff : A.tpr + ok * N + rowoff;
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double x[kRowE];
#pragma unroll
        for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(v[r]);
        wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : ar.to_raw(x[r]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 x[kRowE];
#pragma unroll
        for (int r = 0; r < kRowE; ++r) x[r] = v[r];
        wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : ar.to_raw(x[r]);
    }
    if (valid) store_rowA(dst, lane, v);
}

} // namespace

// =======================================================================================================
// Launchers (the forms, grids and per-engine passes of a launch: ks_launch.h, k3_geometry)
// =======================================================================================================
void launch_k3(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, const u64 *key, K3Part part, const K3Fuse *fuse, int n_split, u64 *split_part,
               int n_split_u64, const KsGroups *groups, u64 g_op_offset)
{
    if (groups && (n_split > 1 || (fuse && fuse->ta))) throw std::runtime_error("grouped keys: the 8-wave rotation instantiations only");
    if (n_split > 1 && !fuse && !split_part) throw std::runtime_error("digit-split K3: unfused launches with a partial-sum buffer only");
    K3Request rq;
    rq.L = L; rq.n_ops = n_ops; rq.part = part; rq.n_split = n_split; rq.n_split_u64 = n_split_u64;
    rq.fuse = fuse != nullptr; rq.tt_lo = fuse ? fuse->tt_lo : 0; rq.tt_hi = fuse ? fuse->tt_hi : 0; rq.rescale = fuse && fuse->cols2;
    rq.grouped = groups != nullptr; rq.group_size = groups ? groups->group_size : 0; rq.sum_out = groups && groups->sum_out; rq.g_op_offset = g_op_offset;
    const K3Geometry G = k3_geometry(ks_launch_dims(env), rq);
    if (!n_ops) return;
    if (fuse && (part != K3_DATA_ONLY || !k3_can_fuse(env))) throw std::runtime_error("fused mod-down: data-prime tiles only");
    K3Args A;
    A.d = buf.d; A.c2n = buf.c2n; A.key = key; A.t = buf.t; A.tp = buf.tp; A.tpr = buf.tpr;
    A.n_ops = n_ops; A.L = L; A.K = env.K; A.logn1 = env.logn1; A.ckks = env.scheme == 2;
    A.cols = fuse ? fuse->cols : nullptr; A.c01 = fuse ? fuse->c01 : nullptr; A.c01_item_stride = fuse ? fuse->c01_item_stride : 0;
    A.cols2 = fuse ? fuse->cols2 : nullptr; A.out2 = fuse ? fuse->out : nullptr;
    A.c1_mode = fuse ? fuse->c1_mode : 0; A.c1_src = fuse ? fuse->c1_src : nullptr;
    A.gsrc = fuse ? fuse->gsrc : nullptr; A.gperm = fuse ? fuse->gperm : nullptr; A.gsrc_op_offset = fuse ? fuse->gsrc_op_offset : 0;
    if ((A.c1_mode == 4 || A.c1_mode == 5) && (!A.gsrc || (!groups && !A.gperm))) throw std::runtime_error("gathered rotation: the input slab and its permutation are needed");
    if (A.c1_mode == 5 && !A.c1_src) throw std::runtime_error("gathered rotation with addend: the addend rows are needed");
    A.ta = fuse ? fuse->ta : nullptr; A.tb = fuse ? fuse->tb : nullptr; A.tix = fuse ? fuse->tix : Indexer{}; A.t_op_offset = fuse ? fuse->t_op_offset : 0;
    if (fuse && fuse->raw_tail) { // the rescale's divided-out prime: operand-formed sums, inverse row pass, raw rows (no floor step)
        if (!fuse->ta || fuse->tt_hi != fuse->tt_lo + 1 || groups) throw std::runtime_error("raw tail: one prime of a ct x ct multiply");
        A.tpr = fuse->raw_tail;
    }
    A.fc = env.floor_consts;
    A.part = split_part;
    A.n_q = G.n_q;
    A.keyq_offset = (u64)env.Ltop * 2 * env.K * env.N; // the quotient array follows the key in the same allocation
    A.keyq = key ? key + A.keyq_offset : nullptr;
    A.groups = groups ? *groups : KsGroups{}; A.g_op_offset = g_op_offset;
    K3Args AP[2] = {A, A};
    for (int i = 0; i < G.n_pend; ++i) {
        const K3Pass &P = G.pend[i];
        copy_list(AP[i].tt_list, AP[i].n_tt, P.tt_list);
        std::copy(P.q_slot, P.q_slot + P.tt_list.n, AP[i].q_slot);
        AP[i].n_split = P.n_split; AP[i].og_per_block = P.og_per_block; AP[i].og_stride = P.og_stride;
    }
    const K3Pass *const pend = G.pend;
    const hipStream_t st3 = env.stream;
    const bool tensor = fuse && fuse->ta, raw_tail = fuse && fuse->raw_tail; // (raw_tail: one prime, so one engine and no dual launch)
    if (G.form == K3Form::Dual) { // latency shape
        const unsigned ny = (unsigned)std::max(pend[0].n_split, pend[1].n_split);
        hipLaunchKernelGGL(k_k3_dual, dim3(pend[0].g + pend[1].g, ny), dim3(64), 0, st3, AP[0], AP[1], pend[1].g, env.primes);
        return;
    }
    if (G.form == K3Form::Dual8) {
        const dim3 gd(pend[0].g + pend[1].g);
#define HE355_K3D8(F, T, G_)                                                                                                                  \
    do {                                                                                                                                      \
        if (pend[1].waves == 4) hipLaunchKernelGGL((k_k3_dual8<F, T, G_, 4>), gd, dim3(512), 0, st3, AP[0], AP[1], pend[1].g, env.primes);     \
        else hipLaunchKernelGGL((k_k3_dual8<F, T, G_, 8>), gd, dim3(512), 0, st3, AP[0], AP[1], pend[1].g, env.primes);                        \
    } while (0)
        if (groups) { if (fuse) HE355_K3D8(true, false, true); else HE355_K3D8(false, false, true); }
        else if (tensor) HE355_K3D8(true, true, false);
        else if (fuse) HE355_K3D8(true, false, false);
        else HE355_K3D8(false, false, false);
#undef HE355_K3D8
        return;
    }
    for (int i = 0; i < G.n_pend; ++i) {
        const K3Args &AA = AP[i];
        const unsigned g = pend[i].g;
        const bool f64 = pend[i].f64;
        KernelProbe *pr = f64 && pend[i].waves == 8 ? env.probe : nullptr;
        int slot = -1;
        if (pr && pr->used < KernelProbe::kCap) {
            slot = pr->used++;
            if (slot >= pr->created) {
                (void)hipEventCreate(&pr->start[slot]);
                (void)hipEventCreate(&pr->stop[slot]);
                pr->created = slot + 1;
            }
            pr->ops += n_ops;
            (void)hipEventRecord(pr->start[slot], env.stream);
        }
        if (pend[i].waves == 1) {
            const dim3 gd(g, (unsigned)AA.n_split);
            if (f64) hipLaunchKernelGGL((k_k3<ArF64, 1>), gd, dim3(64), 0, st3, AA, env.primes);
            else hipLaunchKernelGGL((k_k3<ArU64, 1>), gd, dim3(64), 0, st3, AA, env.primes);
        } else if (pend[i].waves == 4) { // (u64 engine, small grid)
            if (groups && fuse) hipLaunchKernelGGL((k_k3<ArU64, 4, true, false, true>), dim3(g), dim3(256), 0, st3, AA, env.primes);
            else if (groups) hipLaunchKernelGGL((k_k3<ArU64, 4, false, false, true>), dim3(g), dim3(256), 0, st3, AA, env.primes);
            else if (raw_tail) hipLaunchKernelGGL((k_k3<ArU64, 4, false, true>), dim3(g), dim3(256), 0, st3, AA, env.primes);
            else if (tensor) hipLaunchKernelGGL((k_k3<ArU64, 4, true, true>), dim3(g), dim3(256), 0, st3, AA, env.primes);
            else if (fuse) hipLaunchKernelGGL((k_k3<ArU64, 4, true>), dim3(g), dim3(256), 0, st3, AA, env.primes);
            else hipLaunchKernelGGL((k_k3<ArU64, 4>), dim3(g), dim3(256), 0, st3, AA, env.primes);
        } else if (groups) {
            if (f64 && fuse) hipLaunchKernelGGL((k_k3<ArF64, 8, true, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (f64) hipLaunchKernelGGL((k_k3<ArF64, 8, false, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (fuse) hipLaunchKernelGGL((k_k3<ArU64, 8, true, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else hipLaunchKernelGGL((k_k3<ArU64, 8, false, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
        } else if (f64) {
            if (raw_tail) hipLaunchKernelGGL((k_k3<ArF64, 8, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (tensor) hipLaunchKernelGGL((k_k3<ArF64, 8, true, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (fuse) hipLaunchKernelGGL((k_k3<ArF64, 8, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else hipLaunchKernelGGL((k_k3<ArF64, 8>), dim3(g), dim3(512), 0, st3, AA, env.primes);
        } else {
            if (raw_tail) hipLaunchKernelGGL((k_k3<ArU64, 8, false, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (tensor) hipLaunchKernelGGL((k_k3<ArU64, 8, true, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else if (fuse) hipLaunchKernelGGL((k_k3<ArU64, 8, true>), dim3(g), dim3(512), 0, st3, AA, env.primes);
            else hipLaunchKernelGGL((k_k3<ArU64, 8>), dim3(g), dim3(512), 0, st3, AA, env.primes);
        }
        if (slot >= 0) (void)hipEventRecord(pr->stop[slot], env.stream);
    }
    // (the inverse row pass of the special-prime sums, and of every prime's sums for BFV, happened in the kernel's epilogue)
}

void launch_k3_combine(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, int n_split, const u64 *split_part, int n_split_u64)
{
    if (n_split_u64 <= 0) n_split_u64 = n_split;
    if (!n_ops) return;
    K3CombineArgs A;
    A.part = split_part; A.t = buf.t; A.tpr = buf.tpr; A.n_ops = n_ops; A.n_split = n_split; A.n_split_u64 = n_split_u64; A.L = L; A.K = env.K; A.logn1 = env.logn1;
    A.ckks = env.scheme == 2;
    hipLaunchKernelGGL(k_k3_combine, dim3(k3_combine_grid(ks_launch_dims(env), L, n_ops)), dim3(kBlock), 0, env.stream, A, env.primes);
}

} // namespace HE355_KNS
} // namespace he355
