// he355_kernels.hip — hand-written HIP kernels for gfx950 (CDNA4), the two families every call shares: the RNS negacyclic NTT's row and
// column passes over a PolyView, and the streaming element-wise kernels (add / sub, plaintext operands, the dyadic tensor, sums, moves).
// The other families have a file each around the same shared text (kernel_common.inc): the key switch's K1, K2 and floor step
// (he355_kernels_ks.hip), its key product K3 (he355_kernels_k3.hip), the BEHZ multiply and the coefficient-form BFV key-switch tail
// (he355_kernels_behz.hip), the ring-in-LDS key switch (he355_kernels_lds.hip), the hoisted rotations, the client side, ...
//
// Work decomposition (one residue polynomial = N = N1 x 1024 coefficients):
//   * row kernels   : one 64-lane WAVE owns one 1024-element row, 16 elements per lane in VGPRs, the ten
//                     stages run 4+4+2 in registers with two register/lane transposes between them (ntt_core.h),
//                     each an exchange through the wave's own LDS region; a workgroup is four such waves (four
//                     rows of the same residue) and 34 KiB of LDS.
//   * column kernels: one LANE owns one stride-1024 column (N1 <= 32 values in VGPRs); twiddles of a column
//                     pass are wave-uniform, so they come through scalar loads.
// Global accesses are coalesced: layout A reads/writes 512 contiguous bytes per wave instruction, layout C
// moves 16 B per lane (two dwordx4 per 32-byte lane segment; a quad of lanes covers one 128-byte line).
// Reference semantics implemented here: SEAL Evaluator::{add, multiply (CKKS), relinearize_inplace,
// rescale_to_next_inplace, rotate_vector} as called from the reference's src/benchmarks/ckks/*.cpp and
// src/engine/seal_context.cpp (see include/he355.h for the call-site map).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <stdexcept>
#include <type_traits>

#include "he355_kernels.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels.hip is compiled once per form of the u64 engine: -DHE355_KNS=ks_shoup -DHE355_U64_FOLD=0 and -DHE355_KNS=ks_fold -DHE355_U64_FOLD=1 (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// =======================================================================================================
// Generic transforms over a PolyView
// =======================================================================================================
template <class Ar>
__device__ __forceinline__ void rows_fwd_job(const PrimeDev &P, u64 *row, bool in_raw, u32 rowbase, int lane, u64 *lds, bool valid)
{
    const Ar ar = make_ar(P, (Ar *)nullptr);
    typename Ar::T x[kRowE];
    u64 v[kRowE];
    load_rowA(row, lane, v);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) x[r] = in_raw ? ar.from_raw(v[r]) : ar.from_canon(v[r]);
    wave_rows_fwd(ar, tw_table(gtw(P.fwd), rowbase), lane, lds, x);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = ar.to_canon(x[r]);
    if (valid) store_rowC(row, lane, v);
}

__global__ void __launch_bounds__(kBlock) k_rows_fwd(PolyView view, const PrimeDev *primes, u64 total_jobs, int logn1, int in_raw)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << logn1;
    u64 job = (u64)blockIdx.x * kWaves + wave;
    bool valid = job < total_jobs;
    if (!valid) job = total_jobs - 1;
    const u32 a = (u32)(job & (n1 - 1));
    const u64 pj = job >> logn1;
    const int p = (int)(pj % view.polys_per_item);
    const u64 item = pj / view.polys_per_item;
    int prime = view.prime_of[p];
    if (prime == 255) { valid = false; prime = 0; }
    u64 *row = view.base + item * view.item_stride + ((u64)p << (logn1 + kRowLog)) + ((u64)a << kRowLog);
    const PrimeDev &P = primes[prime];
    if (P.f64) rows_fwd_job<ArF64>(P, row, in_raw != 0, n1 + a, lane, lds[wave], valid);
    else rows_fwd_job<ArU64>(P, row, in_raw != 0, n1 + a, lane, lds[wave], valid);
}

template <class Ar>
__device__ __forceinline__ void rows_inv_job(const PrimeDev &P, const u64 *src, u64 *dst, bool last, u32 rowbase, int lane, u64 *lds, bool valid)
{
    const Ar ar = make_ar(P, (Ar *)nullptr);
    typename Ar::T x[kRowE];
    u64 v[kRowE];
    load_rowC(src, lane, v);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(v[r]);
    wave_rows_inv(ar, P, last, rowbase, lane, lds, x);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : ar.to_raw(x[r]);
    if (valid) store_rowA(dst, lane, v);
}

__global__ void __launch_bounds__(kBlock) k_rows_inv(PolyView view, const PrimeDev *primes, u64 total_jobs, int logn1)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << logn1;
    u64 job = (u64)blockIdx.x * kWaves + wave;
    bool valid = job < total_jobs;
    if (!valid) job = total_jobs - 1;
    const u32 a = (u32)(job & (n1 - 1));
    const u64 pj = job >> logn1;
    const int p = (int)(pj % view.polys_per_item);
    const u64 item = pj / view.polys_per_item;
    int prime = view.prime_of[p];
    if (prime == 255) { valid = false; prime = 0; }
    u64 *row = view.base + item * view.item_stride + ((u64)p << (logn1 + kRowLog)) + ((u64)a << kRowLog);
    const PrimeDev &P = primes[prime];
    if (P.f64) rows_inv_job<ArF64>(P, row, row, logn1 == 0, n1 + a, lane, lds[wave], valid);
    else rows_inv_job<ArU64>(P, row, row, logn1 == 0, n1 + a, lane, lds[wave], valid);
}

// inverse row pass of one selected residue per poly into a compact tail buffer
__global__ void __launch_bounds__(kBlock) k_rows_inv_select(const u64 *src, u64 src_poly_stride, u64 *tail, const PrimeDev *primes, int prime,
                                                            u64 total_jobs, int logn1)
{
    __shared__ u64 lds[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << logn1;
    u64 job = (u64)blockIdx.x * kWaves + wave;
    bool valid = job < total_jobs;
    if (!valid) job = total_jobs - 1;
    const u32 a = (u32)(job & (n1 - 1));
    const u64 poly = job >> logn1;
    const u64 *s = src + poly * src_poly_stride + ((u64)a << kRowLog);
    u64 *d = tail + (poly << (logn1 + kRowLog)) + ((u64)a << kRowLog);
    const PrimeDev &P = primes[prime];
    if (P.f64) rows_inv_job<ArF64>(P, s, d, logn1 == 0, n1 + a, lane, lds[wave], valid);
    else rows_inv_job<ArU64>(P, s, d, logn1 == 0, n1 + a, lane, lds[wave], valid);
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_cols_fwd(PolyView view, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 pj = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int p = (int)(pj % view.polys_per_item);
    const u64 item = pj / view.polys_per_item;
    const int prime = view.prime_of[p];
    if (prime == 255) return;
    u64 *poly = view.base + item * view.item_stride + ((u64)p << (LOGN1 + kRowLog));
    const PrimeDev &P = primes[prime];
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(poly[(a << kRowLog) + col]);
        col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) poly[(a << kRowLog) + col] = ar.to_raw(x[a]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = poly[(a << kRowLog) + col];
        col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
        for (int a = 0; a < N1; ++a) poly[(a << kRowLog) + col] = x[a];
    }
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_cols_inv(PolyView view, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 pj = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int p = (int)(pj % view.polys_per_item);
    const u64 item = pj / view.polys_per_item;
    const int prime = view.prime_of[p];
    if (prime == 255) return;
    u64 *poly = view.base + item * view.item_stride + ((u64)p << (LOGN1 + kRowLog));
    const PrimeDev &P = primes[prime];
    if (P.f64) {
        const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(poly[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) poly[(a << kRowLog) + col] = ar.to_canon(x[a]);
    } else {
        const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = poly[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(P.inv), P.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) poly[(a << kRowLog) + col] = ar.to_canon(x[a]);
    }
}

// =======================================================================================================
// Element-wise kernels (HBM-bound): 16 bytes per lane per access
// =======================================================================================================
// Evaluator::add / sub: one thread = 2 coefficients of one residue polynomial of one result.
__global__ void __launch_bounds__(kBlock) k_addsub(const u64 *a, const u64 *b, u64 *out, Indexer ix, const PrimeDev *primes, int L, int polys,
                                                   int logN, u64 n_results, int sub)
{
    const u64 pairs_per_poly = (u64)1 << (logN - 1);
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 pp = gid >> (logN - 1);            // (result, poly)
    const u64 e2 = gid & (pairs_per_poly - 1);   // pair index inside the residue polynomial
    const u64 r = pp / polys;
    if (r >= n_results) return;
    const int p = (int)(pp % polys);
    const u64 q = primes[p % L].q;
    const u64 ct = (u64)polys << logN;
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(a + idx_a(ix, r) * ct + ((u64)p << logN))[e2];
    const ulonglong2 y = reinterpret_cast<const ulonglong2 *>(b + idx_b(ix, r) * ct + ((u64)p << logN))[e2];
    ulonglong2 z;
    if (sub) { z.x = submod(x.x, y.x, q); z.y = submod(x.y, y.y, q); }
    else { z.x = addmod(x.x, y.x, q); z.y = addmod(x.y, y.y, q); }
    reinterpret_cast<ulonglong2 *>(out + r * ct + ((u64)p << logN))[e2] = z;
}

// Evaluator::multiply_plain (mode 0: every polynomial times the NTT-form plaintext) and Evaluator::add_plain, CKKS
// (mode 1: plaintext added to c0, the other polynomials copied).  One thread = 2 coefficients of one residue polynomial.
__global__ void __launch_bounds__(kBlock) k_plain_op(const u64 *ct, const u64 *pt, u64 *out, Indexer ix, const PrimeDev *primes, int L, int size, int logN,
                                                     u64 n_results, int mode)
{
    const u64 pairs_per_poly = (u64)1 << (logN - 1);
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 pp = gid >> (logN - 1);
    const u64 e2 = gid & (pairs_per_poly - 1);
    const int polys = size * L;
    const u64 r = pp / polys;
    if (r >= n_results) return;
    const int p = (int)(pp % polys), i = p % L;
    const PrimeDev &P = primes[i];
    const u64 ctn = (u64)polys << logN;
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(ct + idx_a(ix, r) * ctn + ((u64)p << logN))[e2];
    ulonglong2 z = x;
    if (mode == 0 || p < L) {
        const ulonglong2 y = reinterpret_cast<const ulonglong2 *>(pt + (idx_b(ix, r) * L + i) * ((u64)1 << logN))[e2];
        if (mode == 1) {
            z.x = addmod(x.x, y.x, P.q); z.y = addmod(x.y, y.y, P.q);
        } else if (P.f64) {
            const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
            z.x = ar.dy_out(ar.dy_mul(ar.dy_in(x.x), ar.dy_in(y.x))); z.y = ar.dy_out(ar.dy_mul(ar.dy_in(x.y), ar.dy_in(y.y)));
        } else {
            const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
            z.x = ar.dy_mul(x.x, y.x); z.y = ar.dy_mul(x.y, y.y);
        }
    }
    reinterpret_cast<ulonglong2 *>(out + r * ctn + ((u64)p << logN))[e2] = z;
}

// CKKS mod_switch_to (ciphertexts, NTT-form plaintexts): keep the first L_to residues of every polynomial.
// in [n_polys][L][N] -> out [n_polys][L_to][N]; one thread = 2 coefficients.
__global__ void __launch_bounds__(kBlock) k_drop_residues(const u64 *in, u64 *out, int L, int L_to, int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 pp = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    const u64 poly = pp / L_to;
    if (poly >= n_polys) return;
    const int i = (int)(pp % L_to);
    reinterpret_cast<ulonglong2 *>(out + ((poly * L_to + i) << logN))[e2] = reinterpret_cast<const ulonglong2 *>(in + ((poly * L + i) << logN))[e2];
}

// Sum of n ciphertexts (the add_inplace accumulation of collapseCKKS, seal_context.cpp:401): out = sum_r in[r].
// One thread = 2 coefficients of one residue polynomial of the result; it walks the n terms.
// blockIdx.y + c_first = result c of n_out: out[c] = (accumulate ? out[c] : 0) + sum_r in[r * n_out + c] (n_out = 1: the sum of a run of ciphertexts;
// n_out > 1: the sums over the inner index of a matrix product's terms, he355_bfv_multiply_relin_accumulate)
__global__ void __launch_bounds__(kBlock) k_sum_cts(const u64 *in, u64 *out, const PrimeDev *primes, int L, int polys, int logN, u64 n_terms, int accumulate,
                                                    u64 n_out, u64 c_first)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    if (p >= (u64)polys) return;
    const u64 c = c_first + blockIdx.y;
    const u64 q = primes[p % L].q;
    const u64 ctn = (u64)polys << logN;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(out + c * ctn + (p << logN)) + e2;
    ulonglong2 s = accumulate ? *po : make_ulonglong2(0, 0);
    for (u64 r = 0; r < n_terms; ++r) {
        const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(in + (r * n_out + c) * ctn + (p << logN))[e2];
        s.x = addmod(s.x, x.x, q); s.y = addmod(s.y, x.y, q);
    }
    *po = s;
}

// Sum over the groups of a grouped launch: out[c] (+)= sum_g mult[g] * in[g * n_cts + c] (mult: how many rotation steps end at trie node g;
// he355_rotate_sum).  One thread = 2 coefficients of one residue polynomial of one result ciphertext; it walks the groups.
__global__ void __launch_bounds__(kBlock) k_sum_groups(const u64 *in, u64 *out, const u32 *mult, const PrimeDev *primes, int L, int polys, int logN, u64 n_cts,
                                                       u32 n_groups)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 cp = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    const u64 c = cp / polys;
    if (c >= n_cts) return;
    const int p = (int)(cp % polys);
    const u64 q = primes[p % L].q;
    const u64 ctn = (u64)polys << logN;
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(out + c * ctn + ((u64)p << logN)) + e2;
    ulonglong2 s = *po;
    // four groups' loads in flight per lane (the counts are wave-uniform: scalar loads, uniform branches); every word is read once: non-temporal
    typedef unsigned long long v2u __attribute__((ext_vector_type(2)));
    const v2u *pin = reinterpret_cast<const v2u *>(in + c * ctn + ((u64)p << logN)) + e2;
    const u64 gstride = (n_cts * ctn) >> 1;
    for (u32 g = 0; g < n_groups; g += 4) {
        u32 m[4];
        v2u x[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = g + k < n_groups ? mult[g + k] & ~kGroupKeepBit : 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (m[k]) x[k] = __builtin_nontemporal_load(pin + (u64)(g + k) * gstride);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            for (u32 r = 0; r < m[k]; ++r) { s.x = addmod(s.x, x[k].x, q); s.y = addmod(s.y, x[k].y, q); }
    }
    *po = s;
}

// Gather / scatter of whole ciphertexts by an index list held in the kernel arguments (rotate_each groups the ciphertexts
// that need the same Galois element): gather: dst[g] = src[idx[g]]; scatter: dst[idx[g]] = src[g].  16 B per lane.
struct MoveList {
    uint32_t idx[kMoveListCap];
};
__global__ void __launch_bounds__(kBlock) k_move_cts(u64 *dst, const u64 *src, MoveList list, u64 pairs_per_ct, int scatter)
{
    const u64 g = blockIdx.y;
    const u64 e2 = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (e2 >= pairs_per_ct) return;
    const u64 i = list.idx[g];
    const u64 s = (scatter ? g : i) * pairs_per_ct + e2, d = (scatter ? i : g) * pairs_per_ct + e2;
    reinterpret_cast<ulonglong2 *>(dst)[d] = reinterpret_cast<const ulonglong2 *>(src)[s];
}

// Evaluator::multiply, CKKS, size 2 x 2 -> 3 (dyadic tensor).  One thread = 2 coefficients of one residue.
template <class Ar>
__device__ __forceinline__ void mul3_pair(const Ar &ar, const ulonglong2 a0, const ulonglong2 a1, const ulonglong2 b0, const ulonglong2 b1,
                                          ulonglong2 &c0, ulonglong2 &c1, ulonglong2 &c2)
{
    typename Ar::T x0 = ar.dy_in(a0.x), x1 = ar.dy_in(a1.x), y0 = ar.dy_in(b0.x), y1 = ar.dy_in(b1.x);
    c0.x = ar.dy_out(ar.dy_mul(x0, y0));
    c1.x = ar.dy_out(ar.dy_add(ar.dy_mul(x0, y1), ar.dy_mul(x1, y0)));
    c2.x = ar.dy_out(ar.dy_mul(x1, y1));
    x0 = ar.dy_in(a0.y); x1 = ar.dy_in(a1.y); y0 = ar.dy_in(b0.y); y1 = ar.dy_in(b1.y);
    c0.y = ar.dy_out(ar.dy_mul(x0, y0));
    c1.y = ar.dy_out(ar.dy_add(ar.dy_mul(x0, y1), ar.dy_mul(x1, y0)));
    c2.y = ar.dy_out(ar.dy_mul(x1, y1));
}

__global__ void __launch_bounds__(kBlock) k_mul3(const u64 *a, const u64 *b, u64 *out, Indexer ix, const PrimeDev *primes, int L, int logN,
                                                 u64 n_results)
{
    const u64 pairs_per_poly = (u64)1 << (logN - 1);
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 ri = gid >> (logN - 1);
    const u64 e2 = gid & (pairs_per_poly - 1);
    const u64 r = ri / L;
    if (r >= n_results) return;
    const int i = (int)(ri % L);
    const u64 poly = (u64)1 << logN, P1 = (u64)L << logN;
    const u64 *pa = a + idx_a(ix, r) * 2 * P1 + i * poly, *pb = b + idx_b(ix, r) * 2 * P1 + i * poly;
    const ulonglong2 a0 = reinterpret_cast<const ulonglong2 *>(pa)[e2], a1 = reinterpret_cast<const ulonglong2 *>(pa + P1)[e2];
    const ulonglong2 b0 = reinterpret_cast<const ulonglong2 *>(pb)[e2], b1 = reinterpret_cast<const ulonglong2 *>(pb + P1)[e2];
    ulonglong2 c0, c1, c2;
    const PrimeDev &P = primes[i];
    if (P.f64) mul3_pair(make_ar(P, (ArF64 *)nullptr), a0, a1, b0, b1, c0, c1, c2);
    else mul3_pair(make_ar(P, (ArU64 *)nullptr), a0, a1, b0, b1, c0, c1, c2);
    u64 *po = out + r * 3 * P1 + i * poly;
    reinterpret_cast<ulonglong2 *>(po)[e2] = c0;
    reinterpret_cast<ulonglong2 *>(po + P1)[e2] = c1;
    reinterpret_cast<ulonglong2 *>(po + 2 * P1)[e2] = c2;
}

// Sum over the inner dimension of size-3 dyadic tensors: out(i,j) = sum_k a(i,k) (x) b(k,j) — the multiply / add_inplace
// loop of the CipherBatchAxis workloads (ckks cipherbatchaxis .cpp:404-420) kept in registers: 4 reads per term, 3 writes
// per result.  One thread = 2 coefficients of one residue of one result.
template <class Ar>
__device__ __forceinline__ void mul3_acc_pair(const Ar &ar, u64 q, const u64 *pa, const u64 *pb, u64 a_step, u64 b_step, u64 P1, u64 e2, int inner,
                                              ulonglong2 &s0, ulonglong2 &s1, ulonglong2 &s2)
{
    s0 = s1 = s2 = make_ulonglong2(0, 0);
    for (int k = 0; k < inner; ++k, pa += a_step, pb += b_step) {
        const ulonglong2 a0 = reinterpret_cast<const ulonglong2 *>(pa)[e2], a1 = reinterpret_cast<const ulonglong2 *>(pa + P1)[e2];
        const ulonglong2 b0 = reinterpret_cast<const ulonglong2 *>(pb)[e2], b1 = reinterpret_cast<const ulonglong2 *>(pb + P1)[e2];
        ulonglong2 c0, c1, c2;
        mul3_pair(ar, a0, a1, b0, b1, c0, c1, c2);
        s0.x = addmod(s0.x, c0.x, q); s0.y = addmod(s0.y, c0.y, q);
        s1.x = addmod(s1.x, c1.x, q); s1.y = addmod(s1.y, c1.y, q);
        s2.x = addmod(s2.x, c2.x, q); s2.y = addmod(s2.y, c2.y, q);
    }
}

__global__ void __launch_bounds__(kBlock) k_mul3_acc(const u64 *a, const u64 *b, u64 *out, const PrimeDev *primes, int L, int logN, u64 rows, u64 cols,
                                                     int inner, u64 a_stride_i, u64 a_stride_k, u64 b_stride_k, u64 b_stride_j)
{
    const u64 pairs_per_poly = (u64)1 << (logN - 1);
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 ri = gid >> (logN - 1);
    const u64 e2 = gid & (pairs_per_poly - 1);
    const u64 r = ri / L;
    if (r >= rows * cols) return;
    const int i = (int)(ri % L);
    const u64 poly = (u64)1 << logN, P1 = (u64)L << logN, ct = 2 * P1;
    const u64 *pa = a + (r / cols) * a_stride_i * ct + i * poly, *pb = b + (r % cols) * b_stride_j * ct + i * poly;
    ulonglong2 s0, s1, s2;
    const PrimeDev &P = primes[i];
    if (P.f64) mul3_acc_pair(make_ar(P, (ArF64 *)nullptr), P.q, pa, pb, a_stride_k * ct, b_stride_k * ct, P1, e2, inner, s0, s1, s2);
    else mul3_acc_pair(make_ar(P, (ArU64 *)nullptr), P.q, pa, pb, a_stride_k * ct, b_stride_k * ct, P1, e2, inner, s0, s1, s2);
    u64 *po = out + r * 3 * P1 + i * poly;
    reinterpret_cast<ulonglong2 *>(po)[e2] = s0;
    reinterpret_cast<ulonglong2 *>(po + P1)[e2] = s1;
    reinterpret_cast<ulonglong2 *>(po + 2 * P1)[e2] = s2;
}

} // namespace

// =======================================================================================================
// Launchers
// =======================================================================================================
void launch_rows_fwd(const KernelEnv &env, const PolyView &v, u32 n_items) // the row half of launch_ntt_forward (raw, or canonical when N = 1024, -> NTT form)
{
    const u64 jobs = ((u64)n_items * v.polys_per_item) << env.logn1;
    if (!jobs) return;
    hipLaunchKernelGGL(k_rows_fwd, dim3(blocks_for(jobs, kWaves)), dim3(kBlock), 0, env.stream, v, env.primes, jobs, env.logn1, env.logn1 > 0 ? 1 : 0);
}
void launch_rows_inv(const KernelEnv &env, const PolyView &v, u32 n_items) // the row half of launch_ntt_inverse (NTT form -> raw; N = 1024: coefficients)
{
    const u64 jobs = ((u64)n_items * v.polys_per_item) << env.logn1;
    if (!jobs) return;
    hipLaunchKernelGGL(k_rows_inv, dim3(blocks_for(jobs, kWaves)), dim3(kBlock), 0, env.stream, v, env.primes, jobs, env.logn1);
}
void launch_cols_fwd(const KernelEnv &env, const PolyView &v, u32 n_items) // the column half of launch_ntt_forward (canonical -> raw)
{
    const u64 polys = (u64)n_items * v.polys_per_item;
    if (!polys || env.logn1 == 0) return;
    const unsigned g = (unsigned)(polys * 4);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_cols_fwd<decltype(n1)::value>, dim3(g), dim3(kBlock), 0, env.stream, v, env.primes); });
}
void launch_cols_inv(const KernelEnv &env, const PolyView &v, u32 n_items) // the column half of launch_ntt_inverse (raw -> coefficients)
{
    const u64 polys = (u64)n_items * v.polys_per_item;
    if (!polys || env.logn1 == 0) return;
    const unsigned g = (unsigned)(polys * 4);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_cols_inv<decltype(n1)::value>, dim3(g), dim3(kBlock), 0, env.stream, v, env.primes); });
}
void launch_ntt_forward(const KernelEnv &env, const PolyView &v, u32 n_items)
{
    launch_cols_fwd(env, v, n_items);
    launch_rows_fwd(env, v, n_items);
}
void launch_ntt_inverse(const KernelEnv &env, const PolyView &v, u32 n_items)
{
    launch_rows_inv(env, v, n_items);
    launch_cols_inv(env, v, n_items);
}

void launch_addsub(const KernelEnv &env, int L, int size, u64 n_results, const u64 *a, const u64 *b, Indexer ix, u64 *out, bool sub)
{
    if (!n_results) return;
    const int logN = env.logn1 + kRowLog, polys = size * L;
    const u64 threads = (n_results * polys) << (logN - 1);
    hipLaunchKernelGGL(k_addsub, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, a, b, out, ix, env.primes, L, polys, logN, n_results,
                       sub ? 1 : 0);
}

void launch_plain_op(const KernelEnv &env, int L, int size, u64 n_results, const u64 *ct, const u64 *pt, Indexer ix, u64 *out, int mode)
{
    if (!n_results) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_results * size * L) << (logN - 1);
    hipLaunchKernelGGL(k_plain_op, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, ct, pt, out, ix, env.primes, L, size, logN, n_results, mode);
}
void launch_drop_residues(const KernelEnv &env, int L, int L_to, u64 n_polys, const u64 *in, u64 *out)
{
    if (!n_polys) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_polys * L_to) << (logN - 1);
    hipLaunchKernelGGL(k_drop_residues, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, in, out, L, L_to, logN, n_polys);
}
void launch_sum_cts(const KernelEnv &env, int L, int size, u64 n_terms, const u64 *in, u64 *out, u64 n_out, bool accumulate)
{
    const int logN = env.logn1 + kRowLog;
    const u64 threads = ((u64)size * L) << (logN - 1);
    for (u64 c0 = 0; c0 < n_out; c0 += 65535) { // gridDim.y holds 65535 results
        const unsigned ny = (unsigned)std::min<u64>(65535, n_out - c0);
        hipLaunchKernelGGL(k_sum_cts, dim3(blocks_for(threads, kBlock), ny), dim3(kBlock), 0, env.stream, in, out, env.primes, L, size * L, logN, n_terms,
                           accumulate ? 1 : 0, n_out, c0);
    }
}

void launch_sum_groups(const KernelEnv &env, int L, u64 n_cts, u32 n_groups, const u64 *in, const u32 *d_mult, u64 *out)
{
    if (!n_cts || !n_groups) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_cts * 2 * L) << (logN - 1);
    hipLaunchKernelGGL(k_sum_groups, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, in, out, d_mult, env.primes, L, 2 * L, logN, n_cts, n_groups);
}

void launch_move_cts(const KernelEnv &env, u64 *dst, const u64 *src, const uint32_t *idx, u64 n, u64 elems_per_ct, bool scatter)
{
    const u64 pairs = elems_per_ct / 2;
    for (u64 off = 0; off < n; off += kMoveListCap) {
        const u64 m = std::min<u64>(kMoveListCap, n - off);
        MoveList list;
        for (u64 g = 0; g < m; ++g) list.idx[g] = idx[off + g];
        // gather: compact rows [off, off+m) of dst; scatter: compact rows [off, off+m) of src
        hipLaunchKernelGGL(k_move_cts, dim3(blocks_for(pairs, kBlock), (unsigned)m), dim3(kBlock), 0, env.stream, scatter ? dst : dst + off * elems_per_ct,
                           scatter ? src + off * elems_per_ct : src, list, pairs, scatter ? 1 : 0);
    }
}

void launch_mul3_acc(const KernelEnv &env, int L, u64 rows, u64 cols, int inner, const u64 *a, u64 a_stride_i, u64 a_stride_k, const u64 *b,
                     u64 b_stride_k, u64 b_stride_j, u64 *out)
{
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (rows * cols * (u64)L) << (logN - 1);
    hipLaunchKernelGGL(k_mul3_acc, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, a, b, out, env.primes, L, logN, rows, cols, inner,
                       a_stride_i, a_stride_k, b_stride_k, b_stride_j);
}

void launch_mul3(const KernelEnv &env, int L, u64 n_results, const u64 *a, const u64 *b, Indexer ix, u64 *out)
{
    if (!n_results) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_results * L) << (logN - 1);
    hipLaunchKernelGGL(k_mul3, dim3(blocks_for(threads, kBlock)), dim3(kBlock), 0, env.stream, a, b, out, ix, env.primes, L, logN, n_results);
}

void launch_rows_inv_select(const KernelEnv &env, int prime, u64 n_polys, const u64 *src, u64 src_poly_stride, u64 *tail)
{
    if (!n_polys) return;
    const u64 jobs = n_polys << env.logn1;
    hipLaunchKernelGGL(k_rows_inv_select, dim3(rows_inv_select_grid(ks_launch_dims(env), n_polys)), dim3(kBlock), 0, env.stream, src, src_poly_stride, tail,
                       env.primes, prime, jobs, env.logn1);
}

// (the client-side kernels -- encryption, decryption, encoders, key generation -- and their launchers: he355_kernels_client.hip)
} // namespace HE355_KNS
} // namespace he355
