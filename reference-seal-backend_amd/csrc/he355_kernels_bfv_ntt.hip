// he355_kernels_bfv_ntt.hip -- the NTT-form BFV plaintext inner product: out(i, j) = sum_k ct(i, k) (.) pt(k, j), the multiply_plain +
// add_inplace loop of a plaintext matrix x encrypted vector (he355_bfv_multiply_plain_accumulate).  The per-coefficient arithmetic is
// bfv_mac_core.h (host-compilable: tests/csim_bfv_mac runs the same text on the CPU).
//
//   k_bfv_plain_mac<SIZE, TR, TC>   streaming; a lane owns two coefficients (16 B per access, as k_mul3_acc) of one residue of a TR x TC
//                        tile of results, all SIZE polynomials of each: per inner index it loads TR * SIZE ciphertext words and TC plaintext
//                        words and feeds TR * TC * SIZE sums -- a ciphertext word serves TC columns, a plaintext word TR rows and the SIZE
//                        polynomials of a ciphertext.  The products are summed unreduced in 128 bits and reduced once per run
//                        (bfv_mac_run: 256 terms under a 60-bit prime).  Every prime takes this integer path, those the fp64 engine owns
//                        included: ArF64 sums for them measured -7 % at one shape, +10 % at another and nothing elsewhere, for 36-40 more
//                        registers (profiles/bfv_ntt_form.txt; tools/patches/bfv_plain_mac_f64_engine.patch).  A long row of results
//                        streams at 5.1-5.7 TB/s of compulsory bytes (HBM-bound); a 2 x 2 tile is bound by VALU issue.
//                        Tiles: 1 x 1 (a single row AND column: no tile to pay for), 1 x 4, 4 x 1, 2 x 2, 1 x 2, 2 x 1 (launch_bfv_plain_mac); edge tiles
//                        clamp their loads to the last row / column and do not store what lies outside.  Blocks that share operands
//                        (the tiles of one (residue, coefficient block)) are neighbours in the grid, so they run at the same time and a
//                        word several tiles need is in the caches when the second one asks.
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "he355_kernels.h"
#include "bfv_mac_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_ntt.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

constexpr int kBlock = 256;

struct BfvMacArgs {
    const u64 *ct, *pt;
    u64 *out;
    u64 rows, cols;
    u64 ct_stride_i, ct_stride_k, pt_stride_k, pt_stride_j; // in ciphertexts / plaintexts
    u32 inner, tiles, tiles_c, pairs_blocks;                // tiles = tiles_r * tiles_c; pairs_blocks = N / 2 / kBlock
    int L, logN;
    u32 run[kMaxPrimes]; // bfv_mac_run of prime i
};

template <int SIZE, int TR, int TC>
__global__ void __launch_bounds__(kBlock) k_bfv_plain_mac(BfvMacArgs A, const PrimeDev *primes)
{
    // block = (residue i, coefficient block, tile), the tile fastest
    const u32 tile = blockIdx.x % A.tiles, rest = blockIdx.x / A.tiles;
    const u32 eb = rest % A.pairs_blocks;
    const int i = (int)(rest / A.pairs_blocks);
    const u64 e2 = (u64)eb * kBlock + threadIdx.x;
    const u64 r0 = (u64)(tile / A.tiles_c) * TR, c0 = (u64)(tile % A.tiles_c) * TC;
    const u64 N = (u64)1 << A.logN, LN = (u64)A.L << A.logN, ctn = SIZE * LN;
    const ModU64 m = bfv_modu(primes[i]);
    const u64 run = A.run[i];

    const ulonglong2 *pc[TR], *pp[TC];
#pragma unroll
    for (int a = 0; a < TR; ++a) {
        const u64 row = r0 + a < A.rows ? r0 + a : A.rows - 1;
        pc[a] = reinterpret_cast<const ulonglong2 *>(A.ct + row * A.ct_stride_i * ctn + (u64)i * N) + e2;
    }
#pragma unroll
    for (int b = 0; b < TC; ++b) {
        const u64 col = c0 + b < A.cols ? c0 + b : A.cols - 1;
        pp[b] = reinterpret_cast<const ulonglong2 *>(A.pt + col * A.pt_stride_j * LN + (u64)i * N) + e2;
    }
    const u64 step_c = A.ct_stride_k * ctn / 2, step_p = A.pt_stride_k * LN / 2, poly = LN / 2; // in 16-byte words

    u128 acc[TR][TC][SIZE][2];
#pragma unroll
    for (int a = 0; a < TR; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b)
#pragma unroll
            for (int s = 0; s < SIZE; ++s) acc[a][b][s][0] = acc[a][b][s][1] = 0;

    // two inner indices' loads in flight where there is no tile (few registers, nothing but the streams to wait for); a tile's own loads are enough
    constexpr int kUnroll = TR * TC == 1 ? 2 : 1;
    u64 k = 0, take = run;
    while (k < A.inner) {
        const u64 end = A.inner - k < take ? A.inner : k + take;
#pragma unroll kUnroll
        for (; k < end; ++k) {
            ulonglong2 x[TR][SIZE], y[TC];
#pragma unroll
            for (int a = 0; a < TR; ++a)
#pragma unroll
                for (int s = 0; s < SIZE; ++s) x[a][s] = pc[a][k * step_c + s * poly];
#pragma unroll
            for (int b = 0; b < TC; ++b) y[b] = pp[b][k * step_p];
#pragma unroll
            for (int a = 0; a < TR; ++a)
#pragma unroll
                for (int b = 0; b < TC; ++b)
#pragma unroll
                    for (int s = 0; s < SIZE; ++s) {
                        bfv_mac_add(acc[a][b][s][0], x[a][s].x, y[b].x);
                        bfv_mac_add(acc[a][b][s][1], x[a][s].y, y[b].y);
                    }
        }
        if (k < A.inner) {
#pragma unroll
            for (int a = 0; a < TR; ++a)
#pragma unroll
                for (int b = 0; b < TC; ++b)
#pragma unroll
                    for (int s = 0; s < SIZE; ++s) {
                        bfv_mac_fold(acc[a][b][s][0], m);
                        bfv_mac_fold(acc[a][b][s][1], m);
                    }
        }
        take = run - 1;
    }
#pragma unroll
    for (int a = 0; a < TR; ++a)
#pragma unroll
        for (int b = 0; b < TC; ++b) {
            if (r0 + a >= A.rows || c0 + b >= A.cols) continue;
            ulonglong2 *po = reinterpret_cast<ulonglong2 *>(A.out + ((r0 + a) * A.cols + c0 + b) * ctn + (u64)i * N) + e2;
#pragma unroll
            for (int s = 0; s < SIZE; ++s) po[s * poly] = make_ulonglong2(bfv_mac_reduce(acc[a][b][s][0], m), bfv_mac_reduce(acc[a][b][s][1], m));
        }
}

template <int SIZE, int TR, int TC> void launch_tile(const KernelEnv &env, BfvMacArgs &A)
{
    const u64 tiles_r = (A.rows + TR - 1) / TR, tiles_c = (A.cols + TC - 1) / TC;
    const u64 blocks = tiles_r * tiles_c * A.pairs_blocks * (u64)A.L;
    if (tiles_r * tiles_c > 0x7fffffffull || blocks > 0x7fffffffull) throw std::invalid_argument("he355_bfv_multiply_plain_accumulate: too many results for one launch");
    A.tiles = (u32)(tiles_r * tiles_c);
    A.tiles_c = (u32)tiles_c;
    hipLaunchKernelGGL((k_bfv_plain_mac<SIZE, TR, TC>), dim3((unsigned)blocks), dim3(kBlock), 0, env.stream, A, env.primes);
}

} // namespace

void launch_bfv_plain_mac(const KernelEnv &env, int L, int size, u64 rows, u64 cols, u64 inner, const u64 *ct, u64 ct_stride_i, u64 ct_stride_k, const u64 *pt,
                          u64 pt_stride_k, u64 pt_stride_j, u64 *out)
{
    if (!rows || !cols) return;
    if (L < 1 || L > kMaxPrimes || inner < 1 || inner > 0x7fffffffull) throw std::invalid_argument("he355_bfv_multiply_plain_accumulate: level or inner dimension out of range");
    BfvMacArgs A{};
    A.ct = ct; A.pt = pt; A.out = out; A.rows = rows; A.cols = cols;
    A.ct_stride_i = ct_stride_i; A.ct_stride_k = ct_stride_k; A.pt_stride_k = pt_stride_k; A.pt_stride_j = pt_stride_j;
    A.inner = (u32)inner; A.L = L; A.logN = env.logn1 + kRowLog;
    A.pairs_blocks = (u32)((((u64)1 << A.logN) / 2) / kBlock);
    for (int i = 0; i < L; ++i) {
        A.run[i] = (u32)bfv_mac_run(env.prime_q[i]);
        if (A.run[i] < 2) throw std::invalid_argument("he355_bfv_multiply_plain_accumulate: prime too wide for a 128-bit sum");
    }
    // The tile, from the registers a lane has (tools/kres.py: no scratch, no spill, at most 140 VGPRs) and the words a tile saves: a TR x TC
    // tile loads TR * size + TC words per inner index for TR * TC * size products.  Sizes 1 and 2 keep four results per lane: 2 x 2 where both
    // sides have two or more, 1 x 4 for a single row; for a single column the only shared word is the plaintext's: 4 x 1 at size 1, 2 x 1 at
    // size 2 (4 x 1 there holds 188 registers to read 2.25 instead of 2.5 words per row and term).  Size 3 keeps two results, along the
    // columns where there are any (four size-3 results need more than 256 registers).  A strip of four over fewer than three results would
    // idle half of it: those shapes, and a single row AND column, run the 1 x 1 instantiation and pay for no tile.
    const bool wide = cols >= 3, tall = rows >= 3;
    switch (size) {
    case 1:
        if (rows >= 2 && cols >= 2) launch_tile<1, 2, 2>(env, A);
        else if (rows == 1 && wide) launch_tile<1, 1, 4>(env, A);
        else if (cols == 1 && tall) launch_tile<1, 4, 1>(env, A);
        else launch_tile<1, 1, 1>(env, A);
        break;
    case 2:
        if (rows >= 2 && cols >= 2) launch_tile<2, 2, 2>(env, A);
        else if (rows == 1 && wide) launch_tile<2, 1, 4>(env, A);
        else if (cols == 1 && rows >= 2) launch_tile<2, 2, 1>(env, A);
        else launch_tile<2, 1, 1>(env, A);
        break;
    case 3:
        if (cols >= 2) launch_tile<3, 1, 2>(env, A);
        else if (rows >= 2) launch_tile<3, 2, 1>(env, A);
        else launch_tile<3, 1, 1>(env, A);
        break;
    default: throw std::invalid_argument("ciphertext size must be 1..3");
    }
}

} // namespace HE355_KNS
} // namespace he355
