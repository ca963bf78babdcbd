// he355_kernels_ks.hip -- the hybrid key switch around its key product (DESIGN.md "Key-switch pipeline"): what runs before k_k3
// (he355_kernels_k3.hip) and what finishes the mod-down and the rescale behind it.
//
//   k_k1, k_k1_dual            K1: (multiply | take ct3 | Galois-permute) and the inverse row pass of the key-switch target
//   k_k2n, k_k2n_dual          K2 (body: k2n_body.inc): per (op, digit, column) the rest of the inverse transform, the lift to every key
//                              prime and the forward column pass into the digit slab
//   k_floor_colsn              floor step, column half: the source residue's corrections under every target prime
//   k_floor_rows, _dual        floor step, row half: (sums - NTT(corrections)) * s^-1 (+ addend), optionally into the next step's source
//
// K2 and the floor column pass share their store path and target pipeline (poly_rsrc, store_word_rows, split_mask, load_colw16); the
// twiddle staging K1 and the floor row pass share with k_k3 is kernel_common.inc's.  Grids and engine splits: ks_launch.h.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <type_traits>

#include "he355_kernels.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_ks.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// =======================================================================================================
// K1: (multiply | take ct3 | Galois-permute) + inverse row pass of the key-switch target
// =======================================================================================================
constexpr int K1_MUL_C2 = 3; // k_k1 instantiation of K1_MUL with no_c01 (its own register allocation: the full tensor keeps three waves per SIMD)
struct K1Args {
    const u64 *addend; // GALOIS mode, optional: [n][2][L][N] added to the rotated ciphertext (c0' + addend0, addend1); null: (c0', 0)
    const u64 *a, *b;
    Indexer ix;
    const uint32_t *perm;
    u64 *c01; u64 c01_item_stride;
    u64 *c2n, *c2r;
    u64 n_ops, op_offset;
    int L, logn1, mode;
    int no_c1;                 // K1_GALOIS: polynomial 1 of c01 (zeros / the addend's) is left to the fused k_k3 (K3Fuse::c1_mode)
    int no_c0n;                // K1_GALOIS, no addend: the permuted c0 is not written either (the fused k_k3 gathers it from the input: c1_mode 4)
    int n_i;                   // residues handled by this launch (one arithmetic engine per launch)
    unsigned char i_list[64];
    KsGroups groups;           // K1_GALOIS, grouped launch (group_size > 0): op's source ciphertext and permutation table come from its group
};

// The two operand rows of a K1_MUL_C2 row job.  The throughput shape requests them before it stages the block's twiddles (k_k1): they need
// none, and their way from HBM then runs beside the staging instead of behind its barrier.  (K1_MUL's four rows stay where they are:
// held across the staging they cost its instantiations 30 registers and with them the third wave per SIMD.)
struct K1RowsC2 {
    u64 a1[kRowE], b1[kRowE];
};
__device__ __forceinline__ void k1_load_rows_c2(const K1Args &A, u64 op, int i, u32 a_row, int lane, K1RowsC2 &R)
{
    const u64 N = (u64)(1u << A.logn1) << kRowLog, P1 = (u64)A.L * N;
    const u64 roff = (u64)i * N + ((u64)a_row << kRowLog);
    const u64 r = A.op_offset + op;
    load_rowC(A.a + (idx_a(A.ix, r) * 2 + 1) * P1 + roff, lane, R.a1);
    load_rowC(A.b + (idx_b(A.ix, r) * 2 + 1) * P1 + roff, lane, R.b1);
}

template <class Ar, int MODE, class ITW = int>
__device__ __forceinline__ void k1_job(const K1Args &A, const PrimeDev &P, u64 op, int i, u32 a_row, int lane, u64 *lds, bool valid, const ITW *staged = nullptr,
                                       const K1RowsC2 *rows_c2 = nullptr) // rows_c2 (K1_MUL_C2): the operand rows, requested by the caller
{
    typedef typename Ar::T T;
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog, P1 = (u64)A.L * N;
    const u64 roff = (u64)i * N + ((u64)a_row << kRowLog);
    u64 *c0p = A.c01 + op * A.c01_item_stride + roff;
    u64 *c1p = c0p + P1;
    u64 *c2np = A.c2n + op * P1 + roff;
    u64 *c2rp = A.c2r + op * P1 + roff;
    T x[kRowE];
    u64 v0[kRowE], v1[kRowE];
    if (MODE == K1_MUL || MODE == K1_MUL_C2) {
        const u64 r = A.op_offset + op;
        const u64 *pa = A.a + idx_a(A.ix, r) * 2 * P1 + roff, *pb = A.b + idx_b(A.ix, r) * 2 * P1 + roff;
        u64 a0[kRowE], a1[kRowE], b0[kRowE], b1[kRowE];
        u64 v2[kRowE];
        if (MODE == K1_MUL_C2) { // only the key-switch target c2 = a1 b1, through the inverse row pass (c0, c1 are computed by the fused k_k3 from the operands): half the reads, a quarter of the writes
#pragma unroll
            for (int r2 = 0; r2 < kRowE; ++r2) x[r2] = ar.dy_mul(ar.dy_in(rows_c2->a1[r2]), ar.dy_in(rows_c2->b1[r2])); // the product as it is (fp64 engine: centred lazy, |x| < q): nothing here reads the canonical integer
            // (no c2n row either: the fused k_k3 of a ct x ct multiply forms a1 b1 itself, from the rows it reads for c0, c1)
        } else {
        load_rowC(pa, lane, a0); load_rowC(pa + P1, lane, a1);
        load_rowC(pb, lane, b0); load_rowC(pb + P1, lane, b1);
#pragma unroll
        for (int r2 = 0; r2 < kRowE; ++r2) {
            const T x0 = ar.dy_in(a0[r2]), x1 = ar.dy_in(a1[r2]), y0 = ar.dy_in(b0[r2]), y1 = ar.dy_in(b1[r2]);
            v0[r2] = ar.dy_out(ar.dy_mul(x0, y0));
            v1[r2] = ar.dy_out(ar.dy_add(ar.dy_mul(x0, y1), ar.dy_mul(x1, y0)));
            v2[r2] = ar.dy_out(ar.dy_mul(x1, y1));
            x[r2] = ar.from_canon(v2[r2]);
        }
        if (valid) { store_rowC(c0p, lane, v0); store_rowC(c1p, lane, v1); store_rowC(c2np, lane, v2); }
        }
    } else if (MODE == K1_CT3) {
        const u64 *pa = A.a + (A.op_offset + op) * 3 * P1 + roff;
        u64 v2[kRowE];
        load_rowC(pa + 2 * P1, lane, v2);
#pragma unroll
        for (int r2 = 0; r2 < kRowE; ++r2) x[r2] = ar.from_canon(v2[r2]);
        if (!A.no_c1) { // (no_c1: the fused k_k3 reads c0, c1 and the NTT-form c2 from the size-3 ciphertext itself, K3Fuse::c1_mode 3)
            load_rowC(pa, lane, v0); load_rowC(pa + P1, lane, v1);
            if (valid) { store_rowC(c0p, lane, v0); store_rowC(c1p, lane, v1); store_rowC(c2np, lane, v2); }
        }
    } else { // K1_GALOIS: out[idx] = in[perm[idx]] on both polys; c1 := 0; key-switch target = permuted c1
        u64 src_ct = A.op_offset + op;
        const uint32_t *perm = A.perm;
        if (A.groups.group_size) { // (wave-uniform) the op's group names its source block and its Galois element
            const u32 gop = (u32)(A.op_offset + op), grp = gop / A.groups.group_size;
            src_ct = (u64)A.groups.src_block[grp] * A.groups.group_size + gop % A.groups.group_size;
            perm = A.groups.perm[grp];
        }
        const u64 *p0 = A.a + src_ct * 2 * P1 + (u64)i * N;
        const uint32_t *pm = perm + ((u64)a_row << kRowLog);
        u64 v2[kRowE];
        // The permutation of an NTT-form polynomial maps a row ONTO one source row (the low logn1 + 1 bits of an element's exponent are its
        // row's alone, and so are those of g times it: Params::galois_perm_ntt checks it), so the wave reads that row the way it reads any
        // row -- 16 bytes per lane, every line once -- into its exchange buffer and permutes there: sixteen 8-byte reads per lane at
        // addresses of its own were sixty-four cache lines per instruction for the texture path, and what k_k1 spent its time on.
        {
            const u64 *srow = p0 + (u64)(__builtin_amdgcn_readfirstlane(pm[0]) & ~(u32)(kRowN - 1));
            u32 pl[kRowE];
#pragma unroll
            for (int r2 = 0; r2 < kRowE; ++r2) pl[r2] = lds_pad((int)(pm[elemC(lane, r2)] & (u32)(kRowN - 1)));
            u64 t[kRowE];
            load_rowC(srow + P1, lane, t);
            lds_store_C(lds, lane, t);
            HE_WAVE_SYNC();
#pragma unroll
            for (int r2 = 0; r2 < kRowE; ++r2) v2[r2] = lds[pl[r2]];
            if (!A.no_c0n) {
                load_rowC(srow, lane, t);
                HE_WAVE_SYNC();
                lds_store_C(lds, lane, t);
                HE_WAVE_SYNC();
#pragma unroll
                for (int r2 = 0; r2 < kRowE; ++r2) v0[r2] = lds[pl[r2]];
            }
            HE_WAVE_SYNC(); // (the inverse row pass writes the buffer next)
#pragma unroll
            for (int r2 = 0; r2 < kRowE; ++r2) {
                if (A.no_c0n) v0[r2] = 0;
                v1[r2] = 0;
                x[r2] = ar.from_canon(v2[r2]);
            }
        }
        if (A.addend && !A.no_c0n) { // out = addend + rotate(in): the ciphertext the key-switched result is added into starts from the addend
            const u64 *ad = A.addend + (A.op_offset + op) * 2 * P1 + roff;
            u64 a0[kRowE];
            load_rowC(ad, lane, a0);
            if (!A.no_c1) load_rowC(ad + P1, lane, v1);
#pragma unroll
            for (int r2 = 0; r2 < kRowE; ++r2) v0[r2] = addmod(v0[r2], a0[r2], P.q);
        }
        if (valid) {
            if (!A.no_c0n) store_rowC(c0p, lane, v0);
            if (!A.no_c1) store_rowC(c1p, lane, v1);
            store_rowC(c2np, lane, v2);
        }
    }
    const bool last = A.logn1 == 0;
    if constexpr (std::is_same<ITW, int>::value) wave_rows_inv(ar, P, last, n1 + a_row, lane, lds, x);
    else wave_rows_inv_tw(ar, *staged, P.inv_w0_scaled, last, lane, lds, x); // the row's inverse twiddles, staged in LDS by the block
#pragma unroll
    for (int r2 = 0; r2 < kRowE; ++r2) v0[r2] = last ? ar.to_canon(x[r2]) : ar.to_raw(x[r2]);
    if (valid) store_rowA(c2rp, lane, v0);
}

// Throughput shape (round 5): a block's four waves take the SAME (residue, row) of four consecutive ciphertexts, so the block stages that
// row's 1023 inverse twiddles in LDS once (8 KiB as doubles for the fp64 engine, 16 KiB for the u64 engine) and every phase of the
// four inverse row passes reads them from there -- before, each wave fetched its 46 entries per lane from the prime's 512 KiB table
// in L2, twice the bytes of the row it transformed, with the latency in front of every phase.  Blocks of one tile are consecutive
// (the tile's twiddle rows and, for rotations, its permutation rows stay in L2).  Grid: n_i * n1 * ceil(n_ops / 4).
template <int MODE, class Ar>
__global__ void __launch_bounds__(kBlock) k_k1(K1Args A, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    constexpr bool kF64 = std::is_same<Ar, ArF64>::value;
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kF64 ? kRowTw * 8 : kRowTw * 16];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 n_opg = (A.n_ops + kWaves - 1) / kWaves;
    const u64 tile = blockIdx.x / n_opg, opg = blockIdx.x % n_opg; // (grid = tiles * n_opg exactly)
    const u32 a_row = (u32)(tile & (n1 - 1));
    const int i = A.i_list[tile >> A.logn1];
    u64 op = opg * kWaves + wave;
    const bool valid = op < A.n_ops;
    if (!valid) op = A.n_ops - 1;
    const PrimeDev &P = primes[i];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    if constexpr (MODE == K1_MUL_C2) {
        // the operand rows are requested first and read behind the barrier: results return in issue order, so the wait for the twiddles
        // covers them too, and the block pays the longer of the two latencies, not their sum
        K1RowsC2 rows;
        k1_load_rows_c2(A, op, i, a_row, lane, rows);
        const auto itw = stage_row_twiddles<Ar, kBlock>(P, ar, n1 + a_row, twl_raw, true);
        __syncthreads();
        k1_job<Ar, MODE>(A, P, op, i, a_row, lane, lds[wave], valid, &itw, &rows);
    } else {
        const auto itw = stage_row_twiddles<Ar, kBlock>(P, ar, n1 + a_row, twl_raw, true);
        __syncthreads();
        k1_job<Ar, MODE>(A, P, op, i, a_row, lane, lds[wave], valid, &itw);
    }
}
// Latency shape: the fp64-engine residues (blocks 0 .. n_f - 1) and the u64-engine residues of one key switch in ONE launch (see k_k3_dual)
template <int MODE, class Ar>
__device__ __forceinline__ void k1_block(const K1Args &A, const PrimeDev *primes, const unsigned bid_x, u64 (*lds)[kLdsRow])
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 total = A.n_ops * A.n_i * n1;
    u64 job = (u64)bid_x * kWaves + wave;
    const bool valid = job < total;
    if (!valid) job = total - 1;
    const u32 a_row = (u32)(job & (n1 - 1));
    const u64 oi = job >> A.logn1;
    const int i = A.i_list[oi % A.n_i];
    const u64 op = oi / A.n_i;
    k1_job<Ar, MODE>(A, primes[i], op, i, a_row, lane, lds[wave], valid);
}
template <int MODE>
__global__ void __launch_bounds__(kBlock) k_k1_dual(K1Args AF, K1Args AU, unsigned n_f, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    if (blockIdx.x < n_f) k1_block<MODE, ArF64>(AF, primes, blockIdx.x, lds);
    else k1_block<MODE, ArU64>(AU, primes, blockIdx.x - n_f, lds);
}

// =======================================================================================================
// K2: per (op, digit j, column): finish the inverse transform, lift to every key prime, forward column pass
// =======================================================================================================
struct K2Args {
    const u64 *c2r;
    u64 src_op_stride;
    u64 *d;
    u64 n_ops;
    int L, K, ckks, src_is_coeff;
    u64 f64_mask; // bit t: key prime t belongs to the fp64 engine
    int n_dig;    // digits handled by this launch (one instantiation per digit width: each gets its own register allocation)
    unsigned char dig_list[64];
    int tsplit;   // the targets of a (digit, column block) are dealt to tsplit blocks (blockIdx.y): latency shape, small grids
};

// What surrounds the butterflies is as lean as the butterflies (round 3; the first form of this kernel spent ~1000 VALU instructions per
// fp64 target and lane for 640 instructions of butterflies, HISTORY.md):
//   * the digit column is held in the form the targets consume: canonical doubles when q_j < 2^52 (every target of the fp64
//     engine then reads it as is; the two u64-engine targets convert back), integers only for a 60-bit digit;
//   * column twiddles come from PrimeDev::colw (bare doubles): 62 scalar registers per target instead of 124;
//   * the first stage reads the digit column and writes the target column (no copy of 32 values per target), the last stage
//     produces the 48-bit patterns directly (BIAS);
//   * every store address is (scalar row base) + (one per-lane 32-bit offset computed once per kernel): the slab pointer of the
//     target is made wave-uniform explicitly, the row bases advance on the scalar unit.
// canonical v of a prime >= 2^52 as a lazy value of the fp64 engine: hi * 2^32 + lo == hi * pow32 + lo (mod q), |result| < q/2 + 2^32 + 1
__device__ __forceinline__ double lift_wide(const ArF64 &ar, u64 v, double pow32)
{
    return ar.mulmod_vv((double)(u32)(v >> 32), pow32) + (double)(u32)v;
}
typedef const __attribute__((address_space(4))) double *cdw_t;
__device__ __forceinline__ cdw_t cdw(const double *p) { return (cdw_t)(unsigned long long)p; }
// Buffer resource over one polynomial's row slots (wave-uniform base made explicit with v_readfirstlane): a store through it is
// buffer_store ... v_off, s[rsrc], s_off offen -- address = base + (scalar row offset) + (per-lane 32-bit offset computed once per
// kernel), no VALU instruction per store.
typedef u32 u32x2_t __attribute__((ext_vector_type(2)));
constexpr u32 kSlotBytes = kRowN * 8; // one row slot of a slab
__device__ __forceinline__ __amdgpu_buffer_rsrc_t poly_rsrc(const void *p, u32 bytes)
{
    const unsigned long long v = (unsigned long long)p;
    const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0, (int)bytes, 0x00020000);
}
// 48-bit pattern rows of one polynomial: row a in slot a, low words at lane offset off4 = 4 * col, high half-words at
// off2h = kPackHiOff + 2 * col
template <int N1> __device__ __forceinline__ void store_pattern_rows(__amdgpu_buffer_rsrc_t dst, u32 off4, u32 off2h, const double x[N1])
{
#pragma unroll
    for (int a = 0; a < N1; ++a) {
        union { u64 u; double d; } c;
        c.d = x[a];
        __builtin_amdgcn_raw_buffer_store_b32((u32)c.u, dst, (int)off4, a * (int)kSlotBytes, 0);
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(c.u >> 32), dst, (int)off2h, a * (int)kSlotBytes, 0);
    }
}
template <int N1> __device__ __forceinline__ void store_word_rows(__amdgpu_buffer_rsrc_t dst, u32 off8, const u64 x[N1])
{
#pragma unroll
    for (int a = 0; a < N1; ++a) {
        u32x2_t v;
        v.x = (u32)x[a]; v.y = (u32)(x[a] >> 32);
        __builtin_amdgcn_raw_buffer_store_b64(v, dst, (int)off8, a * (int)kSlotBytes, 0);
    }
}
// N1 >= 8: the pattern rows of a wave's 64 columns go through a 12 KiB LDS tile (8 KiB of low words, 4 KiB of high half-words,
// row-major) and leave as 16-byte stores: 8 + 4 buffer_store_dwordx4 of 1 KiB per target instead of 32 + 32 stores of 256 / 128 bytes.
// Only the issuing wave touches its tile (wavefront-scope hand-off).  lane_lo / lane_hi: the per-lane byte offsets of the 16-byte
// pieces inside a group of 4 (low plane) / 8 (high plane) rows, wave's column offset included.
typedef u32 u32x4_t __attribute__((ext_vector_type(4)));
template <int N1>
__device__ __forceinline__ void store_pattern_rows_wide(__amdgpu_buffer_rsrc_t dst, unsigned char *tile, int lane, u32 lane_lo, u32 lane_hi, const double x[N1])
{
    static_assert(N1 % 8 == 0, "written for whole groups of 8 rows");
    u32 *lo = reinterpret_cast<u32 *>(tile);
    unsigned short *hi = reinterpret_cast<unsigned short *>(tile + N1 * 256);
#pragma unroll
    for (int a = 0; a < N1; ++a) {
        union { u64 u; double d; } c;
        c.d = x[a];
        lo[a * 64 + lane] = (u32)c.u;
        hi[a * 64 + lane] = (unsigned short)(c.u >> 32);
    }
    HE_WAVE_SYNC();
    const u32x4_t *lo4 = reinterpret_cast<const u32x4_t *>(tile);
    const u32x4_t *hi4 = reinterpret_cast<const u32x4_t *>(tile + N1 * 256);
    // all reads first, into registers of their own (left to itself the scheduler chains read -> wait -> store through one register quad)
    u32x4_t vl[N1 / 4], vh[N1 / 8];
#pragma unroll
    for (int k = 0; k < N1 / 4; ++k) vl[k] = lo4[k * 64 + lane];
#pragma unroll
    for (int k = 0; k < N1 / 8; ++k) vh[k] = hi4[k * 64 + lane];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < N1 / 4; ++k) // 4 rows x 256 bytes per instruction
        __builtin_amdgcn_raw_buffer_store_b128(vl[k], dst, (int)lane_lo, k * 4 * (int)kSlotBytes, 0);
#pragma unroll
    for (int k = 0; k < N1 / 8; ++k) // 8 rows x 128 bytes per instruction
        __builtin_amdgcn_raw_buffer_store_b128(vh[k], dst, (int)lane_hi, k * 8 * (int)kSlotBytes, 0);
    HE_WAVE_SYNC(); // the tile is free again for the next target
}

// Per-target constants come through the constant address space (scalar loads): a vector load of a PrimeDev field would put an
// s_waitcnt vmcnt(0) -- i.e. the full HBM write latency of the previous target's stores -- in front of every target.
// butterflies of a column-pass stage issued together (interleaved dependent chains, ArF64::mulmod_vv_g)
constexpr int kK2G = 2;
// every n_groups-th set bit of mask, starting with the g-th (latency shape: the targets of a column are dealt to n_groups blocks)
__device__ __forceinline__ u64 split_mask(u64 mask, int g, int n_groups)
{
    if (n_groups <= 1) return mask;
    u64 out = 0;
    int r = 0;
    for (u64 m = mask; m; m &= m - 1, ++r)
        if (r % n_groups == g) out |= m & (~m + 1);
    return out;
}
typedef const __attribute__((address_space(4))) PrimeDev *cprime_t;
typedef double d16_t __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(4))) d16_t *cd16_t;
__device__ __forceinline__ d16_t load_colw16(cprime_t cp, int t, int first) { return *(cd16_t)(unsigned long long)&cp[t].colw[first]; }

// Targets of the fp64 engine on the fast path (host-built masks PrimeDev::k2_direct / k2_lift of the digit's prime: the 48-bit row
// format holds the column pass's output).  One iteration per target prime t in `mask` (bit = prime index), software-pipelined
// over the scalar loads: the twiddles of stages 0..3 (entries 0..15) and the modulus constants of the NEXT target are requested
// before the current target's last stage and its stores, the 16 entries of stage 4 at the top of the target, behind stages 0..3 --
// as the compiler places them (one s_load + s_waitcnt lgkmcnt(0) per stage) each target waited five scalar-load latencies.
// DIRECT: the column enters as it is; else it is lifted first (re-centred, or reduced with integers from a 60-bit digit: DF false).
template <int LOGN1, bool DF, bool DIRECT, class Store>
__device__ __forceinline__ void k2n_fast_targets(const K2Args &A, const PrimeDev *primes, int j, u64 op, u64 mask,
                                                 const typename std::conditional<DF, double, u64>::type (&c)[1 << LOGN1], Store store_rows)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    constexpr int LA = LOGN1 < 4 ? LOGN1 : 4; // stages served by entries 0..15
    static_assert(DF || !DIRECT, "an integer digit is always lifted");
    if (!mask) return;
    const cprime_t cp = (cprime_t)(unsigned long long)primes;
    u64 m = mask;
    int t = __builtin_ctzll(m);
    d16_t wa = load_colw16(cp, t, 0);
    double qd = cp[t].qd, qinv = cp[t].qinv;
    // Scalar loads return out of order, so every wait on one is lgkmcnt(0), a wait on all of them.  The waits are therefore placed by
    // hand where nothing young is in flight: here, and before the next target's prefetch below (the stage-4 entries, requested at the
    // top of the target, landed long before); the tile's LDS traffic then covers the prefetch.
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0)
    for (;;) {
        m &= m - 1;
        const int tn = m ? __builtin_ctzll(m) : t;
        d16_t wb = wa;
        if constexpr (LOGN1 == 5) wb = load_colw16(cp, t, 16);
        __builtin_amdgcn_sched_barrier(0);
        ArF64 ar;
        ar.q = qd; ar.qinv = qinv; ar.ninv = 0; ar.ninv_i = 0;
        double x[N1];
        if constexpr (!DIRECT) {
            if constexpr (DF) {
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = ar.renorm(c[a]);
            } else { // a 60-bit digit: hi * (2^32 mod q_t) + lo, one exact fp64 product (lift_wide) instead of a 64-bit Barrett reduction
                const double pow32 = cp[t].pow32;
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = lift_wide(ar, c[a], pow32);
            }
        }
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int gap = N1 >> (s + 1);
            // the stage's N1/2 butterflies, kK2G at a time (interleaved instruction chains)
            constexpr int G = (N1 / 2) % kK2G == 0 ? kK2G : 1;
#pragma unroll
            for (int b0 = 0; b0 < N1 / 2; b0 += G) {
                double X[G], Y[G], W[G], tw[G];
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const int b = b0 + k, a = ((b / gap) * 2 * gap) + (b % gap); // butterfly b of the stage: rows a, a + gap
                    W[k] = wa[(1 << s) + (a / (2 * gap))];
                    if (DIRECT && s == 0) { X[k] = (double)c[a]; Y[k] = (double)c[a + gap]; }
                    else { X[k] = x[a]; Y[k] = x[a + gap]; }
                }
                ar.template mulmod_vv_g<G>(Y, W, tw);
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const int b = b0 + k, a = ((b / gap) * 2 * gap) + (b % gap);
                    if (s == LOGN1 - 1) {
                        const double xb = X[k] + kPackBias;
                        x[a] = xb + tw[k]; x[a + gap] = xb - tw[k];
                    } else {
                        x[a] = X[k] + tw[k]; x[a + gap] = X[k] - tw[k];
                    }
                }
            }
        }
        // the next target's first twiddles and constants: in flight behind the last stage and the stores
        __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): this target's stage-4 entries
        const d16_t wa_n = load_colw16(cp, tn, 0);
        const double qd_n = cp[tn].qd, qinv_n = cp[tn].qinv;
        __builtin_amdgcn_sched_barrier(0);
        const int tt = t == A.K - 1 ? A.L : t;
        const __amdgpu_buffer_rsrc_t dst = poly_rsrc(A.d + ((op * (A.L + 1) + tt) * A.L + j) * N, (u32)N1 * kSlotBytes);
        if constexpr (LOGN1 == 5) {
            constexpr int G = kK2G;
#pragma unroll
            for (int a0 = 0; a0 < N1; a0 += 2 * G) {
                double Y[G], W[G], tw[G];
#pragma unroll
                for (int k = 0; k < G; ++k) { Y[k] = x[a0 + 2 * k + 1]; W[k] = wb[(a0 >> 1) + k]; }
                ar.template mulmod_vv_g<G>(Y, W, tw);
#pragma unroll
                for (int k = 0; k < G; ++k) {
                    const double xb = x[a0 + 2 * k] + kPackBias;
                    x[a0 + 2 * k] = xb + tw[k]; x[a0 + 2 * k + 1] = xb - tw[k];
                }
            }
        }
        if constexpr (LOGN1 == 0) x[0] = (DIRECT ? (double)c[0] : x[0]) + kPackBias;
        __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): the prefetch had the last stage to land; the tile's LDS traffic then waits by count
        store_rows(dst, x);
        if (!m) break;
        t = tn; wa = wa_n; qd = qd_n; qinv = qinv_n;
    }
}

// Targets of the fp64 engine.  DF: the digit's canonical coefficients are held as doubles (q_j < 2^52), else as integers.
template <int LOGN1, bool DF>
__device__ __forceinline__ void k2n_targets_f64(const K2Args &A, const PrimeDev *primes, const PrimeDev &Pj, int j, u64 op,
                                                const typename std::conditional<DF, double, u64>::type (&c)[1 << LOGN1], int col, unsigned char *tile)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    constexpr bool kWide = N1 >= 8;
    const u32 off4 = (u32)col << 2, off2h = ((u32)col << 1) + kPackHiOff;
    const int lane = col & 63;
    const u32 wc = (u32)col & ~63u; // the wave's first column
    const u32 lane_lo = ((u32)lane >> 4) * kSlotBytes + (wc << 2) + (((u32)lane & 15u) << 4);
    const u32 lane_hi = ((u32)lane >> 3) * kSlotBytes + kPackHiOff + (wc << 1) + (((u32)lane & 7u) << 4);
    auto store_rows = [&](__amdgpu_buffer_rsrc_t dst, const double (&x)[N1]) {
        if constexpr (kWide) store_pattern_rows_wide<N1>(dst, tile, lane, lane_lo, lane_hi, x);
        else store_pattern_rows<N1>(dst, off4, off2h, x);
    };
    // this launch's targets by prime index: data primes [0, L) and the special prime, without the digit's own prime (CKKS: that
    // digit is the NTT-form input itself)
    const cprime_t cp = (cprime_t)(unsigned long long)primes;
    u64 level = (A.L >= 64 ? ~(u64)0 : (((u64)1 << A.L) - 1)) | ((u64)1 << (A.K - 1));
    if (A.ckks) level &= ~((u64)1 << j);
    level = split_mask(level, (int)blockIdx.y, A.tsplit);
    const u64 f64_targets = A.f64_mask & level;
    const u64 direct = cp[j].k2_direct & f64_targets, lift = cp[j].k2_lift & f64_targets;
    if constexpr (DF) k2n_fast_targets<LOGN1, DF, true>(A, primes, j, op, direct, c, store_rows);
    k2n_fast_targets<LOGN1, DF, false>(A, primes, j, op, DF ? lift : (lift | direct), c, store_rows);
    // the general path: any lift, results re-centred before they are packed (wider fp64-engine primes)
    for (u64 m = f64_targets & ~(direct | lift); m; m &= m - 1) {
        const int t = __builtin_ctzll(m), tt = t == A.K - 1 ? A.L : t;
        const PrimeDev &Pt = primes[t];
        const __amdgpu_buffer_rsrc_t dst = poly_rsrc(A.d + ((op * (A.L + 1) + tt) * A.L + j) * N, (u32)N1 * kSlotBytes);
        const ArF64 ar = make_ar(Pt, (ArF64 *)nullptr);
        const cdw_t cw = cdw(Pt.colw);
        double x[N1];
        if constexpr (DF) {
            const bool recentre = Pj.q > 2 * Pt.q;
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = recentre ? ar.renorm(c[a]) : c[a];
        } else {
            const ModU64 mt = make_modu(Pt);
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = u52_to_f64(barrett64(c[a], mt));
        }
        col_fwd_w<LOGN1, false>(ar, [&](int a) { return x[a]; }, x, cw, 0.0);
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.renorm(x[a]) + kPackBias;
        store_rows(dst, x);
    }
}
// Targets of the u64 engine, from the digit's canonical coefficients as integers.
template <int LOGN1>
__device__ __forceinline__ void k2n_targets_u64(const K2Args &A, const PrimeDev *primes, const PrimeDev &Pj, int j, u64 op, const u64 (&c)[1 << LOGN1], int col)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    const u32 off8 = (u32)col << 3;
    u64 level = (A.L >= 64 ? ~(u64)0 : (((u64)1 << A.L) - 1)) | ((u64)1 << (A.K - 1));
    if (A.ckks) level &= ~((u64)1 << j);
    level = split_mask(level, (int)blockIdx.y, A.tsplit);
    for (u64 m = ~A.f64_mask & level; m; m &= m - 1) {
        const int t = __builtin_ctzll(m), tt = t == A.K - 1 ? A.L : t;
        const PrimeDev &Pt = primes[t];
        const __amdgpu_buffer_rsrc_t dst = poly_rsrc(A.d + ((op * (A.L + 1) + tt) * A.L + j) * N, (u32)N1 * kSlotBytes);
        const ArU64 ar = make_ar(Pt, (ArU64 *)nullptr);
        u64 x[N1];
        if (Pj.q > Pt.q) {
            const ModU64 mt = make_modu(Pt);
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = barrett64(c[a], mt);
        } else {
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = c[a];
        }
        col_fwd<ArU64, LOGN1>(ar, x, ctw(Pt.fwd));
        store_word_rows<N1>(dst, off8, x);
    }
}

// WIDE: the launch's digits are 60-bit (integers throughout); else below 2^52 (doubles).  Two instantiations instead of one kernel with
// both paths: each gets its own register allocation (one kernel at 168 registers spilled 102 through the wide path's live ranges and
// cost 14.9 ms; at 256 it took 12.4; the pair takes 11.0 + 1.0).  Two or three waves per SIMD make no difference to the narrow
// instantiation any more (11.04 / 11.18 ms): two leave it without spills.
template <int LOGN1, bool WIDE>
__global__ void __launch_bounds__(kBlock, 2) k_k2n(K2Args A, const PrimeDev *primes)
{
#define K2N_BID_X blockIdx.x
#include "k2n_body.inc"
#undef K2N_BID_X
}
// Latency shape: the digits below 2^52 (blocks 0 .. n_n - 1) and the 60-bit digits of one key switch in ONE launch (see k_k3_dual);
// blockIdx.y = target group for both (same tsplit).
template <int LOGN1, bool WIDE>
__device__ __forceinline__ void k2n_body_fn(const K2Args &A, const PrimeDev *primes, const unsigned bid_x)
{
#define K2N_BID_X bid_x
#include "k2n_body.inc"
#undef K2N_BID_X
}
template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_k2n_dual(K2Args AN, K2Args AW, unsigned n_n, const PrimeDev *primes)
{
    if (blockIdx.x < n_n) k2n_body_fn<LOGN1, false>(AN, primes, blockIdx.x);
    else k2n_body_fn<LOGN1, true>(AW, primes, blockIdx.x - n_n);
}

// =======================================================================================================
// Floor step, column half (key-switch mod-down and rescale): finish the inverse transform of the source
// residue, add floor(s/2), reduce into every target prime, subtract floor(s/2), forward column pass.
// =======================================================================================================
struct FloorColsArgs {
    const u64 *src;
    u64 *dst;
    int src_prime, n_tgt, K;
    const FloorConst *fc;
    int tgt_first, dst_ntgt; // targets [tgt_first, tgt_first + n_tgt) of a destination slab laid out for dst_ntgt targets
    // optional (MERGE): an earlier floor step's SOURCE ([n_polys][N], after the inverse row pass, prime src2_prime): its correction is
    // formed here in coefficient form and folded in BEFORE the column pass, delta = delta2 + src2^-1 * delta1 mod q_i, so mod-down and
    // rescale share ONE column pass and ONE row transform per target (both passes are linear) and the earlier correction slab is
    // neither written for these targets nor read back
    const u64 *src2;
    int src2_prime;
    // MERGE, optional: `src` holds the sums of prime src_prime with the earlier correction still in them (k_k3's raw_tail rows: sums scaled
    // by src2^-1, no floor step taken), so the earlier floor step's result under this prime is finished here, once per column and in
    // coefficient form, c' = x - src2^-1 * delta1 mod q_src, before anything reads it
    int sub2;
    u64 f64_mask; // bit i: key prime i belongs to the fp64 engine
    int tsplit;   // latency shape: the targets of a column are dealt to tsplit blocks (blockIdx.y)
};

// canonical coefficients + floor(s/2) of one column of a source residue after its inverse row pass
// SUB (fp64-engine source, LOGN1 > 0): sub[a], an integer double below q_s in magnitude, is taken off each coefficient on the way -- in
// the engine's lazy range, ahead of the one canonicalisation, which then takes floor(s/2) with it too
template <int LOGN1, bool SUB = false>
__device__ __forceinline__ void floor_source_column(const PrimeDev &Ps, const u64 *src, int col, u64 c[1 << LOGN1], const double *sub = nullptr)
{
    constexpr int N1 = 1 << LOGN1;
    static_assert(!SUB || LOGN1 > 0, "the correction rides the fp64 column pass");
    if (LOGN1 == 0) {
        c[0] = src[col];
    } else if (SUB || Ps.f64) {
        const ArF64 ar = make_ar(Ps, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(Ps.inv), Ps.inv_w0_scaled);
        if constexpr (SUB) { // x centred (the last stage's products), |sub| < q, floor(s/2) < q: far inside to_canon's 2^52
            const double half = u52_to_f64(Ps.q >> 1);
#pragma unroll
            for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a] - sub[a] + half);
            return;
        }
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    } else {
        const ArU64 ar = make_ar(Ps, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(Ps.inv), Ps.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    }
    const u64 qs = Ps.q, half = qs >> 1;
#pragma unroll
    for (int a = 0; a < N1; ++a) c[a] = addmod(c[a], half, qs);
}

// The corrections are formed in the target's own engine (round 3; the first form used 64-bit Barrett reductions, HISTORY.md): under an
// fp64-engine target a source residue below 2^52 enters as the double it is (re-centred only where q_s > 2 q_i), a wider one as
// hi * (2^32 mod q_i) + lo, one exact fp64 product (8 instructions instead of ~35 per element for the 60-bit special prime).  Per-target
// constants sit in a small LDS table filled once per block (wave-uniform ds_reads, no scalar registers), the column twiddles come from
// PrimeDev::colw through the same software pipeline as k_k2n's, rows leave through buffer stores whose addresses cost no VALU
// instruction.
struct FcnConsts { // one per target prime, as the fp64 engine wants them
    double half1, half2;   // floor(s/2) mod q_i for the source / the merged earlier source
    double inv2, inv2_i;   // src2^-1 mod q_i and fl(inv2 / q_i)
    double pow32, qd, qinv;
    double recentre;       // bit 0: source 1 needs re-centring (q_s > 2 q_i), bit 1: source 2 does
};

// WIDE1: source 1 is held as integers (q_s >= 2^52), else as doubles
template <int LOGN1, bool MERGE, bool WIDE1>
__device__ __forceinline__ void fcn_targets_f64(const FloorColsArgs &A, const PrimeDev *primes, u64 poly, int col, u64 mask,
                                                const typename std::conditional<WIDE1, u64, double>::type (&c)[1 << LOGN1],
                                                const u64 *park /* [N1][kBlock] when MERGE */, bool wide2, const FcnConsts *ctab)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    constexpr int LA = LOGN1 < 4 ? LOGN1 : 4;
    if (!mask) return;
    const u32 off8 = (u32)col << 3;
    const cprime_t cp = (cprime_t)(unsigned long long)primes;
    u64 m = mask;
    int t = __builtin_ctzll(m);
    d16_t wa = load_colw16(cp, t, 0);
    FcnConsts k = ctab[t];
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0), see k2n_fast_targets
    for (;;) {
        m &= m - 1;
        const int tn = m ? __builtin_ctzll(m) : t;
        d16_t wb = wa;
        if constexpr (LOGN1 == 5) wb = load_colw16(cp, t, 16);
        __builtin_amdgcn_sched_barrier(0);
        ArF64 ar;
        ar.q = k.qd; ar.qinv = k.qinv; ar.ninv = 0; ar.ninv_i = 0;
        const int flags = (int)k.recentre;
        double x[N1];
        // delta2 = [source 1]_{q_i} - floor(s/2)
#pragma unroll
        for (int a = 0; a < N1; ++a) {
            double v;
            if constexpr (WIDE1) v = lift_wide(ar, c[a], k.pow32);
            else v = (flags & 1) ? ar.renorm((double)c[a]) : (double)c[a];
            x[a] = v - k.half1;
        }
        if constexpr (MERGE) { // + src2^-1 * delta1, delta1 = [source 2]_{q_i} - floor(src2/2)
#pragma unroll
            for (int a = 0; a < N1; ++a) {
                const u64 v2 = park[a * kBlock + threadIdx.x];
                double v;
                if (wide2) v = lift_wide(ar, v2, k.pow32);
                else { v = u52_to_f64(v2); if (flags & 2) v = ar.renorm(v); }
                x[a] += ar.mulmod_c(v - k.half2, k.inv2, k.inv2_i);
            }
        }
        // the next target's constants (LDS table): requested here, needed after the stores
        const FcnConsts kn = ctab[tn];
#pragma unroll
        for (int s = 0; s < LA; ++s) {
            const int gap = N1 >> (s + 1);
#pragma unroll
            for (int a = 0; a < N1; ++a) {
                if (a & gap) continue;
                const double tw = ar.mulmod_vv(x[a + gap], wa[(1 << s) + (a / (2 * gap))]);
                const double X = x[a];
                x[a] = X + tw; x[a + gap] = X - tw;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0): the stage-4 entries (and the constants just read)
        const d16_t wa_n = load_colw16(cp, tn, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (LOGN1 == 5) {
#pragma unroll
            for (int a = 0; a < N1; a += 2) {
                const double tw = ar.mulmod_vv(x[a + 1], wb[a >> 1]);
                const double X = x[a];
                x[a] = X + tw; x[a + 1] = X - tw;
            }
        }
        u64 v[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) v[a] = ar.to_raw(x[a]);
        __builtin_amdgcn_s_waitcnt(0xC07F);
        store_word_rows<N1>(poly_rsrc(A.dst + (poly * A.dst_ntgt + t) * N, (u32)N1 * kSlotBytes), off8, v);
        if (!m) break;
        t = tn; wa = wa_n; k = kn;
    }
}

template <int LOGN1, bool MERGE>
__global__ void __launch_bounds__(kBlock, 2) k_floor_colsn(FloorColsArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    const u64 poly = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    __shared__ u64 park[MERGE ? N1 : 1][MERGE ? kBlock : 1];
    __shared__ FcnConsts ctab[kMaxPrimes];
    const PrimeDev &Ps = primes[A.src_prime];
    const u64 qs = Ps.q, qs2 = MERGE ? primes[A.src2_prime].q : 0;
    if ((int)threadIdx.x >= A.tgt_first && (int)threadIdx.x < A.tgt_first + A.n_tgt) { // this block's constants, one thread per target
        const int i = threadIdx.x;
        const PrimeDev &Pi = primes[i];
        FcnConsts k;
        k.half1 = (double)A.fc[A.src_prime * A.K + i].half_mod;
        k.half2 = 0; k.inv2 = 0; k.inv2_i = 0;
        int flags = qs > 2 * Pi.q ? 1 : 0;
        if (MERGE) {
            const FloorConst f2 = A.fc[A.src2_prime * A.K + i];
            k.half2 = (double)f2.half_mod; k.inv2 = f2.inv_d; k.inv2_i = f2.inv_i;
            flags |= qs2 > 2 * Pi.q ? 2 : 0;
        }
        k.pow32 = Pi.pow32; k.qd = Pi.qd; k.qinv = Pi.qinv; k.recentre = (double)flags;
        ctab[i] = k;
    }
    u64 c[N1];
    if constexpr (MERGE) {
        u64 c2[N1];
        floor_source_column<LOGN1>(primes[A.src2_prime], A.src2 + poly * N, col, c2);
#pragma unroll
        for (int a = 0; a < N1; ++a) park[a][threadIdx.x] = c2[a]; // each thread reads back only what it wrote itself
        if (A.sub2) {
            // source 1 still lacks the earlier correction under its own prime: c' = x - src2^-1 * delta1 mod q_src, once per column,
            // delta1 = [source 2]_{q_src} - floor(src2 / 2)
            const FloorConst fs = A.fc[A.src2_prime * A.K + A.src_prime];
            bool done = false;
            if constexpr (LOGN1 > 0) {
                if (Ps.f64) { // in the engine's doubles, folded into the column's one canonicalisation
                    const ArF64 ar = make_ar(Ps, (ArF64 *)nullptr);
                    const double pow32 = Ps.pow32, half2 = (double)fs.half_mod;
                    double d[N1];
#pragma unroll
                    for (int a = 0; a < N1; ++a) d[a] = ar.mulmod_c(lift_wide(ar, c2[a], pow32) - half2, fs.inv_d, fs.inv_i);
                    floor_source_column<LOGN1, true>(Ps, A.src + poly * N, col, c, d);
                    done = true;
                }
            }
            if (!done) { // integers (any prime, either form of the u64 engine)
                floor_source_column<LOGN1>(Ps, A.src + poly * N, col, c);
                const ModU64 ms = make_modu(Ps);
#pragma unroll
                for (int a = 0; a < N1; ++a) {
                    const u64 d1 = submod(qs2 > qs ? barrett64(c2[a], ms) : c2[a], fs.half_mod, qs);
                    c[a] = submod(c[a], mulmod(d1, fs.inv, ms), qs);
                }
            }
        } else {
            floor_source_column<LOGN1>(Ps, A.src + poly * N, col, c);
        }
    } else {
        floor_source_column<LOGN1>(Ps, A.src + poly * N, col, c);
    }
    __syncthreads(); // the constants table
    u64 tgt = ((A.tgt_first + A.n_tgt >= 64 ? ~(u64)0 : (((u64)1 << (A.tgt_first + A.n_tgt)) - 1))) & ~(((u64)1 << A.tgt_first) - 1);
    tgt = split_mask(tgt, (int)blockIdx.y, A.tsplit);
    const u64 f64t = tgt & A.f64_mask;
    const bool wide2 = MERGE && (qs2 >> 52) != 0;
    if (qs >> 52) {
        fcn_targets_f64<LOGN1, MERGE, true>(A, primes, poly, col, f64t, c, &park[0][0], wide2, ctab);
    } else {
        double cd[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) cd[a] = u52_to_f64(c[a]);
        fcn_targets_f64<LOGN1, MERGE, false>(A, primes, poly, col, f64t, cd, &park[0][0], wide2, ctab);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = f64_to_u52(cd[a]);
    }
    // u64-engine targets: integers throughout
    const u32 off8 = (u32)col << 3;
    for (u64 m = tgt & ~A.f64_mask; m; m &= m - 1) {
        const int i = __builtin_ctzll(m);
        const PrimeDev &Pi = primes[i];
        const u64 qi = Pi.q;
        const u64 half_i = A.fc[A.src_prime * A.K + i].half_mod;
        const ModU64 mi = make_modu(Pi);
        const ArU64 ar = make_ar(Pi, (ArU64 *)nullptr);
        u64 dl[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) dl[a] = submod(qs > qi ? barrett64(c[a], mi) : c[a], half_i, qi);
        if constexpr (MERGE) { // [0,q) + [0,q): a valid lazy input of the column pass
            const FloorConst f2 = A.fc[A.src2_prime * A.K + i];
#pragma unroll
            for (int a = 0; a < N1; ++a) {
                const u64 v2 = park[a][threadIdx.x];
                const u64 d1 = submod(qs2 > qi ? barrett64(v2, mi) : v2, f2.half_mod, qi);
                dl[a] += mul_pre(d1, f2.inv, f2.inv_shoup, qi);
            }
        }
        col_fwd<ArU64, LOGN1>(ar, dl, ctw(Pi.fwd));
        store_word_rows<N1>(poly_rsrc(A.dst + (poly * A.dst_ntgt + i) * N, (u32)N1 * kSlotBytes), off8, dl);
    }
}

// =======================================================================================================
// Floor step, row half: out = (tsrc - NTT(cols)) * s^-1 (+ addend) mod q_i; optional inverse-row-pass tail
// =======================================================================================================
struct FloorRowsDev {
    FloorRowsArgs a;
    const FloorConst *fc;
    u64 n_ops;
    int K, logn1;
    int n_i;
    u32 jobs_per_block; // multiple of kWaves
    unsigned char i_list[64];
};

// (a device function: the latency shape runs both engines' instantiations in one launch, k_floor_rows_dual, on one set of LDS buffers)
template <class Ar, bool TAIL>
__device__ __forceinline__ void floor_rows_block(const FloorRowsDev &A, const PrimeDev *primes, const unsigned bid_x, u64 (*lds)[kLdsRow],
                                                 unsigned char *twl_raw)
{
    typedef typename Ar::T T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    // A block owns one (target prime, row) tile and walks jobs_per_block consecutive (op, poly) jobs of it, one job per
    // wave per step: the row's twiddles are staged in LDS once and every later access is a ds_read.
    const u64 n_jobs = A.n_ops * A.a.n_src;
    const u64 n_jb = (n_jobs + A.jobs_per_block - 1) / A.jobs_per_block;
    const u64 tile = bid_x / n_jb;
    const u64 j_begin = (bid_x % n_jb) * A.jobs_per_block;
    const u64 j_end = j_begin + A.jobs_per_block < n_jobs ? j_begin + A.jobs_per_block : n_jobs;
    const int i = A.i_list[tile >> A.logn1];
    const u32 a_row = (u32)(tile & (n1 - 1));
    const PrimeDev &P = primes[i];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const FloorConst fc = A.fc[A.a.src_prime * A.K + i];
    const u64 rowoff = (u64)a_row << kRowLog;
    const auto twr = stage_row_twiddles<Ar, kBlock>(P, ar, n1 + a_row, twl_raw);
    __syncthreads();
    for (u64 j = j_begin + wave; j < j_end; j += kWaves) { // no block-level synchronisation inside: waves run independently
        const int k = (int)(j % A.a.n_src);
        const u64 op = j / A.a.n_src;
        T x[kRowE];
        u64 v[kRowE];
        load_rowA(A.a.cols + ((op * A.a.n_src + k) * A.a.n_tgt + i) * N + rowoff, lane, v);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) x[r] = ar.from_raw(v[r]);
        wave_rows_fwd(ar, twr, lane, lds[wave], x);
        {
            u64 tv[kRowE], av[kRowE];
            load_rowC(A.a.tsrc + op * A.a.tsrc_op_stride + k * A.a.tsrc_poly_stride + (u64)i * N + rowoff, lane, tv);
            if (A.a.addend) load_rowC(A.a.addend + op * A.a.add_op_stride + k * A.a.add_poly_stride + (u64)i * N + rowoff, lane, av);
#pragma unroll
            for (int r = 0; r < kRowE; ++r) v[r] = ar.floor_fin(tv[r], x[r], fc.inv, fc.inv_shoup, fc.inv_d, fc.inv_i, A.a.addend ? av[r] : 0);
        }
        if (A.a.out) store_rowC(A.a.out + op * A.a.out_op_stride + k * A.a.out_poly_stride + (u64)i * N + rowoff, lane, v);
        if (TAIL) { // this prime is the next floor step's source: start its inverse transform right here
            const bool last = A.logn1 == 0;
#pragma unroll
            for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(v[r]);
            wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
#pragma unroll
            for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : ar.to_raw(x[r]);
            store_rowA(A.a.tail + (op * A.a.n_src + k) * N + rowoff, lane, v);
        }
    }
}
template <class Ar, bool TAIL>
__global__ void __launch_bounds__(kBlock) k_floor_rows(FloorRowsDev A, const PrimeDev *primes)
{
    constexpr bool kF64 = std::is_same<Ar, ArF64>::value;
    __shared__ u64 lds[kWaves][kLdsRow];
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kF64 ? kRowTw * 8 : kRowTw * 16];
    floor_rows_block<Ar, TAIL>(A, primes, blockIdx.x, lds, twl_raw);
}
// Latency shape: the fp64-engine targets (blocks 0 .. n_f - 1) and the u64-engine targets of one floor step in ONE launch (see k_k3_dual)
__global__ void __launch_bounds__(kBlock) k_floor_rows_dual(FloorRowsDev AF, FloorRowsDev AU, unsigned n_f, const PrimeDev *primes)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    __shared__ __attribute__((aligned(16))) unsigned char twl_raw[kRowTw * 16];
    if (blockIdx.x < n_f) floor_rows_block<ArF64, false>(AF, primes, blockIdx.x, lds, twl_raw);
    else floor_rows_block<ArU64, false>(AU, primes, blockIdx.x - n_f, lds, twl_raw);
}

} // namespace

// =======================================================================================================
// Launchers (which launches of a stage run as one kernel for both engines, and every grid below: ks_launch.h)
// =======================================================================================================
void launch_k1(const KernelEnv &env, int L, u64 n_ops, const K1Operands &src, const KsBuffers &buf)
{
    if (!n_ops) return;
    const K1Mode mode = src.mode;
    const u64 *const addend = src.addend;
    const KsGroups *const groups = src.groups;
    const bool no_c01 = src.no_c01, no_c1 = src.no_c1, no_c0n = src.no_c0n;
    if (groups && (mode != K1_GALOIS || addend)) throw std::runtime_error("grouped launch: rotations without addend only");
    if (no_c01 && mode != K1_MUL) throw std::runtime_error("no_c01: the ct x ct multiply only");
    if (no_c1 && mode != K1_GALOIS && mode != K1_CT3) throw std::runtime_error("no_c1: rotations and size-3 inputs only");
    K1Args A;
    A.no_c1 = no_c1 ? 1 : 0;
    if (no_c0n && (mode != K1_GALOIS || !no_c1 || (addend && groups))) throw std::runtime_error("no_c0n: rotations whose polynomial 1 is left to k_k3 only");
    A.no_c0n = no_c0n ? 1 : 0;
    A.groups = groups ? *groups : KsGroups{};
    A.a = src.a; A.b = src.b; A.ix = src.ix; A.perm = src.perm; A.addend = addend;
    A.c01 = buf.c01; A.c01_item_stride = buf.c01_item_stride; A.c2n = buf.c2n; A.c2r = buf.c2r;
    A.n_ops = n_ops; A.op_offset = src.op_offset; A.L = L; A.logn1 = env.logn1; A.mode = (int)mode;
    const bool c2_only = mode == K1_MUL && no_c01;
    const K1Geometry G = k1_geometry(ks_launch_dims(env), L, n_ops, c2_only);
    K1Args AP[2] = {A, A}; // [0]: fp64-engine residues, [1]: u64-engine residues
    for (int pass = 0; pass < 2; ++pass) copy_list(AP[pass].i_list, AP[pass].n_i, G.i_list[pass]);
    const hipStream_t st = env.stream;
    if (G.dual) {
        const dim3 grid(G.dual_grid[0] + G.dual_grid[1]);
        if (mode == K1_MUL) hipLaunchKernelGGL((k_k1_dual<K1_MUL>), grid, dim3(kBlock), 0, st, AP[0], AP[1], G.dual_grid[0], env.primes);
        else if (mode == K1_CT3) hipLaunchKernelGGL((k_k1_dual<K1_CT3>), grid, dim3(kBlock), 0, st, AP[0], AP[1], G.dual_grid[0], env.primes);
        else hipLaunchKernelGGL((k_k1_dual<K1_GALOIS>), grid, dim3(kBlock), 0, st, AP[0], AP[1], G.dual_grid[0], env.primes);
        return;
    }
    for (int pass = 0; pass < 2; ++pass) {
        if (!G.grid[pass]) continue;
        const K1Args &AA = AP[pass];
        const dim3 grid(G.grid[pass]);
        if (pass == 0) {
            if (c2_only) hipLaunchKernelGGL((k_k1<K1_MUL_C2, ArF64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else if (mode == K1_MUL) hipLaunchKernelGGL((k_k1<K1_MUL, ArF64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else if (mode == K1_CT3) hipLaunchKernelGGL((k_k1<K1_CT3, ArF64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else hipLaunchKernelGGL((k_k1<K1_GALOIS, ArF64>), grid, dim3(kBlock), 0, st, AA, env.primes);
        } else {
            if (c2_only) hipLaunchKernelGGL((k_k1<K1_MUL_C2, ArU64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else if (mode == K1_MUL) hipLaunchKernelGGL((k_k1<K1_MUL, ArU64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else if (mode == K1_CT3) hipLaunchKernelGGL((k_k1<K1_CT3, ArU64>), grid, dim3(kBlock), 0, st, AA, env.primes);
            else hipLaunchKernelGGL((k_k1<K1_GALOIS, ArU64>), grid, dim3(kBlock), 0, st, AA, env.primes);
        }
    }
}

void launch_k2(const KernelEnv &env, int L, u64 n_ops, const KsBuffers &buf, const u64 *src, u64 src_op_stride, int tsplit)
{
    if (!n_ops) return;
    const KsLaunchDims dims = ks_launch_dims(env);
    K2Args A;
    A.c2r = src ? src : buf.c2r;
    A.src_op_stride = src ? src_op_stride : (u64)L * env.N;
    A.src_is_coeff = src ? 1 : 0;
    A.d = buf.d; A.n_ops = n_ops; A.L = L; A.K = env.K; A.ckks = env.scheme == 2;
    A.f64_mask = f64_mask(dims);
    const K2Geometry G = k2_geometry(dims, L, n_ops, tsplit);
    K2Args AK[2] = {A, A}; // digits below 2^52, then the 60-bit ones
    for (int wide = 0; wide < 2; ++wide) {
        copy_list(AK[wide].dig_list, AK[wide].n_dig, G.dig_list[wide]);
        AK[wide].tsplit = G.ts[wide];
    }
    if (G.dual) {
        const dim3 gd(G.gx[0] + G.gx[1], (unsigned)G.ts[0]);
        dispatch_logn1<0>(env.logn1, [&](auto n1) {
            hipLaunchKernelGGL((k_k2n_dual<decltype(n1)::value>), gd, dim3(kBlock), 0, env.stream, AK[0], AK[1], G.gx[0], env.primes);
        });
        return;
    }
    for (int wide = 0; wide < 2; ++wide) {
        if (!G.gx[wide]) continue;
        const dim3 gd(G.gx[wide], (unsigned)G.ts[wide]);
        dispatch_logn1<0>(env.logn1, [&](auto n1) {
            constexpr int L1 = decltype(n1)::value;
            if (wide) hipLaunchKernelGGL((k_k2n<L1, true>), gd, dim3(kBlock), 0, env.stream, AK[wide], env.primes);
            else hipLaunchKernelGGL((k_k2n<L1, false>), gd, dim3(kBlock), 0, env.stream, AK[wide], env.primes);
        });
    }
}

void launch_floor_cols(const KernelEnv &env, int src_prime, int n_tgt, u64 n_polys, const u64 *src, u64 *dst, int tgt_first, int dst_ntgt, const u64 *src2,
                       int src2_prime, int tsplit, bool sub2)
{
    if (sub2 && !src2) throw std::runtime_error("floor column pass: the earlier correction comes from the merged source");
    if (!n_polys || n_tgt <= 0) return;
    const FloorColsGrid gc = floor_cols_grid(n_polys, tsplit);
    FloorColsArgs A;
    A.src = src; A.dst = dst; A.src_prime = src_prime; A.n_tgt = n_tgt; A.K = env.K; A.fc = env.floor_consts;
    A.tgt_first = tgt_first; A.dst_ntgt = dst_ntgt > 0 ? dst_ntgt : n_tgt;
    A.src2 = src2; A.src2_prime = src2_prime; A.sub2 = sub2;
    A.tsplit = (int)gc.y;
    const dim3 g(gc.x, gc.y);
    A.f64_mask = f64_mask(ks_launch_dims(env));
    dispatch_logn1<0>(env.logn1, [&](auto n1) {
        constexpr int L1 = decltype(n1)::value;
        if (src2) hipLaunchKernelGGL((k_floor_colsn<L1, true>), g, dim3(kBlock), 0, env.stream, A, env.primes);
        else hipLaunchKernelGGL((k_floor_colsn<L1, false>), g, dim3(kBlock), 0, env.stream, A, env.primes);
    });
}

void launch_floor_rows(const KernelEnv &env, u64 n_ops, const FloorRowsArgs &args)
{
    if (!n_ops) return;
    const FloorRowsGeometry G = floor_rows_geometry(ks_launch_dims(env), n_ops, args.n_tgt, args.n_src, args.tail_prime);
    FloorRowsDev AE[4]; // the (engine, tail) passes
    for (int pass = 0; pass < 4; ++pass) {
        FloorRowsDev &A = AE[pass];
        A.a = args; A.fc = env.floor_consts; A.n_ops = n_ops; A.K = env.K; A.logn1 = env.logn1;
        A.jobs_per_block = G.jobs_per_block;
        copy_list(A.i_list, A.n_i, G.i_list[pass]);
    }
    const hipStream_t st = env.stream;
    if (G.dual) {
        hipLaunchKernelGGL(k_floor_rows_dual, dim3(G.g[0] + G.g[2]), dim3(kBlock), 0, st, AE[0], AE[2], G.g[0], env.primes);
        return;
    }
    if (G.g[0]) hipLaunchKernelGGL((k_floor_rows<ArF64, false>), dim3(G.g[0]), dim3(kBlock), 0, st, AE[0], env.primes);
    if (G.g[1]) hipLaunchKernelGGL((k_floor_rows<ArF64, true>), dim3(G.g[1]), dim3(kBlock), 0, st, AE[1], env.primes);
    if (G.g[2]) hipLaunchKernelGGL((k_floor_rows<ArU64, false>), dim3(G.g[2]), dim3(kBlock), 0, st, AE[2], env.primes);
    if (G.g[3]) hipLaunchKernelGGL((k_floor_rows<ArU64, true>), dim3(G.g[3]), dim3(kBlock), 0, st, AE[3], env.primes);
}

} // namespace HE355_KNS
} // namespace he355
