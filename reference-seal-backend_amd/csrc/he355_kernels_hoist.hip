// he355_kernels_hoist.hip -- hoisted rotations (he355_apply_galois_hoisted, he355_rotate_hoisted, he355_rotate_hoisted_plain_sum): the
// digit lift of c1 runs once per chunk, every Galois element then pays a key product and mod-down under its key permuted by g^-1, and
// one of the finishing kernels here applies sigma_g to (c0 + u0, u1).  The per-element arithmetic is hoist_core.h (host-compilable:
// tests/csim/sim_hoist.cpp runs the same text on the CPU).
//
//   k_key_permute          streaming, once per (element, key install): every residue polynomial of an installed key -- and of the Shoup
//                          quotient block behind it -- with its positions permuted by perm(g^-1).  The installed format is pointwise (doubles
//                          for the fp64-engine residues, integers and per-element quotients for the u64 engine), so moving 64-bit words is
//                          all it takes.  A lane gathers two words and makes one 16-byte store.
//   k_hoist_finish_ntt     one wave per (ciphertext, polynomial, prime, row): the row of a permuted NTT-form polynomial has ONE source row
//                          (Params::galois_perm_ntt), read whole in 16-byte loads -- the key switch's and, for polynomial 0, the input's c0 --
//                          added, permuted through the wave's LDS row and stored in 16-byte stores.  <PLAIN>: times the plaintext's row, the
//                          first element of the sum stores and later ones read-modify-write the output row (one stream, launches in order).
//   k_hoist_acc_qp         the lazy plain sum (he355_rotate_hoisted_plain_sum_lazy): one wave per (ciphertext, polynomial, tile, row), tiles = the
//                          data primes and the special prime.  The key product's ONE source row -- under the special prime k_k3 left it after
//                          its inverse row pass: the wave runs the forward row pass -- permuted through the wave's LDS row, times the plaintext's
//                          row, accumulated in Q P; c0's row goes through the same permutation into the output rows.  ONE mod-down follows.
//   k_hoist_rot_qp         the baby-step/giant-step transform (he355_linear_transform_bsgs): k_hoist_acc_qp<true> without a plaintext -- the key
//                          product's source row, P times c0's folded in for polynomial 0, permuted and stored (a baby term) or added into the
//                          giant accumulator.  k_bsgs_ident: the identity baby, streaming.  k_bsgs_inner: a giant row's inner sum over its used
//                          terms in 128-bit sums (bsgs_core.h), streaming, ciphertext-fastest so that the plaintext rows are re-read from cache.
//   k_plain_extend         streaming (he355_plain_extend_special): the rows of a plaintext copied and its row under the special prime made
//                          from the centred coefficients of row 0; optionally counts the coefficients whose other residues disagree.
//   k_hoist_addend_coeff   streaming, once per chunk (BFV coefficient form): (c0, 0), what launch_bfv_tail_fin adds every element's key
//                          switch into.
//   k_hoist_finish_coeff   streaming: the signed gather of Params::galois_gather_coeff(g) on (c0 + u0, u1); a lane gathers two coefficients
//                          and makes one 16-byte store.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "bsgs_core.h"
#include "he355_kernels.h"
#include "hoist_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_hoist.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// polynomial p < n_polys of dst is polynomial p of src with element e taken from perm[e]
__global__ void __launch_bounds__(kBlock) k_key_permute(const u64 *src, u64 *dst, const uint32_t *perm, int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (logN - 1);
    if (p >= n_polys) return;
    const u32 e2 = (u32)(gid & (((u64)1 << (logN - 1)) - 1));
    const uint2 pe = reinterpret_cast<const uint2 *>(perm)[e2];
    const u64 *s = src + (p << logN);
    reinterpret_cast<ulonglong2 *>(dst + (p << logN))[e2] = make_ulonglong2(s[pe.x], s[pe.y]);
}

struct HoistNttArgs {
    const u64 *u;         // [n_ops][2][L][N]: the key switch of c1 under the permuted key, no addend; null: the identity (out = in, PLAIN's term)
    const u64 *in;        // [n_ops][2][L][N]: the chunk's input ciphertexts (c0 is read)
    const uint32_t *perm; // [N]: Params::galois_perm_ntt(g)
    u64 *out;             // [n_ops][2][L][N]
    const u64 *plain;     // PLAIN: [L][N], shared by the chunk
    u64 n_ops;
    int L, logn1;
    int first;            // PLAIN: the sum starts with this element (out is stored, not read)
};

template <bool PLAIN>
__global__ void __launch_bounds__(kBlock) k_hoist_finish_ntt(HoistNttArgs A, const PrimeDev *primes)
{
    __shared__ u64 lds_all[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u64 *lds = lds_all[wave];
    const u32 n1 = 1u << A.logn1;
    const u64 total = (A.n_ops * 2 * (u64)A.L) << A.logn1;
    const u64 job = (u64)blockIdx.x * kWaves + wave;
    if (job >= total) return; // (the whole wave; waves of a block share nothing)
    const u32 a_row = (u32)(job & (n1 - 1));
    const u64 pi = job >> A.logn1; // (op, polynomial, prime)
    const int i = (int)(pi % (u64)A.L);
    const bool poly0 = ((pi / (u64)A.L) & 1) == 0;
    const u64 N = (u64)n1 << kRowLog;
    const PrimeDev &P = primes[i];
    const u64 q = P.q;
    const uint32_t *pm = A.perm + ((u64)a_row << kRowLog);
    const u64 srow = (u64)hoist_src_row(__builtin_amdgcn_readfirstlane(pm[0])) << kRowLog;
    const u64 base = pi * N; // the same [op][polynomial][prime] layout on every side
    u64 v[kRowE];
    if (!A.u) { // the identity as a term of the plain sum: the input itself, both polynomials
        load_rowC(A.in + base + srow, lane, v);
    } else {
        load_rowC(A.u + base + srow, lane, v);
    }
    if (A.u && poly0) {
        u64 c[kRowE];
        load_rowC(A.in + base + srow, lane, c);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = hoist_join(v[r], c[r], true, q);
    }
    // the output positions this lane stores (layout C: four runs of four neighbours) and where each comes from in the source row
    u32 pl[kRowE];
    {
        const uint32_t *pb = pm + ((lane >> 2) << 6) + ((lane & 3) << 2);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint4 w = *reinterpret_cast<const uint4 *>(pb + (c << 4));
            pl[4 * c + 0] = (u32)lds_pad((int)hoist_src_elem(w.x)); pl[4 * c + 1] = (u32)lds_pad((int)hoist_src_elem(w.y));
            pl[4 * c + 2] = (u32)lds_pad((int)hoist_src_elem(w.z)); pl[4 * c + 3] = (u32)lds_pad((int)hoist_src_elem(w.w));
        }
    }
    lds_store_C(lds, lane, v);
    HE_WAVE_SYNC();
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = lds[pl[r]];
    u64 *orow = A.out + base + ((u64)a_row << kRowLog);
    if constexpr (PLAIN) {
        const ModU64 m = make_modu(P);
        u64 pt[kRowE], acc[kRowE];
        load_rowC(A.plain + (u64)i * N + ((u64)a_row << kRowLog), lane, pt);
        if (A.first) {
#pragma unroll
            for (int r = 0; r < kRowE; ++r) acc[r] = 0;
        } else {
            load_rowC(orow, lane, acc);
        }
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = hoist_plain_term(acc[r], v[r], pt[r], m);
    }
    store_rowC(orow, lane, v);
}

struct HoistAccArgs {
    const u64 *t;         // [n_ops][2][L][N]: one element's key product under the permuted key, data primes, canonical NTT form (KEYED)
    const u64 *tpr;       // [n_ops][2][N]: the same under the special prime AFTER k_k3's inverse row pass (raw rows; coefficients when N = 1024) (KEYED)
    const u64 *in;        // [n_ops][2][L][N]: the chunk's input ciphertexts
    const uint32_t *perm; // [N]: Params::galois_perm_ntt(g) (KEYED)
    const u64 *plain;     // [L + 1][N]: the element's plaintext, row L under the special prime (the identity reads rows 0 .. L - 1)
    u64 *aq;              // [n_ops] x aq_op_stride, [2][L][N] each: the Q part of the accumulator A (KEYED)
    u64 aq_op_stride;
    u64 *ap;              // [n_ops][2][N]: the P part of A (KEYED)
    u64 *out;             // [n_ops][2][L][N]: the accumulator B, the call's output rows
    u64 n_ops;
    int L, K, logn1;
    u64 sp_fix;           // 1024^-1 mod P, what the forward row pass of an unnormalised inverse row pass leaves to divide out; N = 1024: 1
    int first_a;          // A starts with this element (stored, not read)
    int first_b;          // B starts with this term (stored, not read; a keyed first term zeroes polynomial 1 of B)
};
// The special prime's source row back in canonical NTT form, layout C: k_k3 leaves its sums after the inverse row pass (tpr), an
// unnormalised Gentleman-Sande pass of ten stages whose N^-1 waits in the column pass (ntt_core.h: row_inv_A_w<., false>), so the forward
// row pass of the same row returns 1024 times the sums and `fix` = 1024^-1 mod P takes that out.  N = 1024: the inverse row pass was the
// whole transform, N^-1 = 1024^-1 included (bfly_inv_last), and the forward row pass returns the sums themselves (fix = 1, not multiplied).
// The raw words are made canonical first: the forward pass then starts from the range it has after a column pass in either engine.
template <class Ar>
__device__ __forceinline__ void hoist_sp_row(const PrimeDev &P, const u64 *row, bool last, u32 rowbase, int lane, u64 *lds, const ModU64 &m, u64 fix, u64 v[kRowE])
{
    const Ar ar = make_ar(P, (Ar *)nullptr);
    typename Ar::T x[kRowE];
    load_rowA(row, lane, v);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(last ? v[r] : ar.to_canon(ar.from_raw(v[r])));
    wave_rows_fwd(ar, tw_table(gtw(P.fwd), rowbase), lane, lds, x);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : hoist_sp_unscale(ar.to_canon(x[r]), fix, m);
}
// One term of the lazy plain sum.  KEYED: one wave per (ciphertext, polynomial, tile 0 .. L, row): the ONE source row of the key product --
// t for a data prime, tpr through hoist_sp_row for the special prime -- permuted through the wave's LDS row, times the plaintext's row, into A; for polynomial 0
// and a data prime the same wave carries the input's c0 source row through the same permutation into B.  The identity (!KEYED): one wave per
// (ciphertext, polynomial, data prime, row), the input's own row times the plaintext's into B, no permutation.
template <bool KEYED>
__global__ void __launch_bounds__(kBlock) k_hoist_acc_qp(HoistAccArgs A, const PrimeDev *primes)
{
    __shared__ u64 lds_all[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const int tiles = KEYED ? A.L + 1 : A.L;
    const u64 total = (A.n_ops * 2 * (u64)tiles) << A.logn1;
    const u64 job = (u64)blockIdx.x * kWaves + wave;
    if (job >= total) return; // (the whole wave; waves of a block share nothing)
    const u32 a_row = (u32)(job & (n1 - 1));
    const u64 pi = job >> A.logn1; // (op, polynomial, tile)
    const int idx = (int)(pi % (u64)tiles);
    const u64 ok = pi / (u64)tiles, op = ok >> 1; // ok = op * 2 + polynomial
    const bool poly0 = (ok & 1) == 0;
    const u64 N = (u64)n1 << kRowLog, arow = (u64)a_row << kRowLog;
    const PrimeDev &P = primes[hoist_qp_prime(idx, A.L, A.K)];
    const ModU64 m = make_modu(P);
    const u64 ct_off = (ok * (u64)A.L + (u64)idx) * N; // the [op][polynomial][prime] layout of in / t / out (idx < L)
    u64 v[kRowE], pt[kRowE], acc[kRowE];
    load_rowC(A.plain + (u64)idx * N + arow, lane, pt);
    if constexpr (!KEYED) {
        load_rowC(A.in + ct_off + arow, lane, v);
    } else {
        u64 *lds = lds_all[wave];
        const uint32_t *pm = A.perm + arow;
        const u64 srow = (u64)hoist_src_row(__builtin_amdgcn_readfirstlane(pm[0])) << kRowLog;
        const bool data = idx < A.L;
        if (data) {
            load_rowC(A.t + ct_off + srow, lane, v);
        } else { // (wave-uniform)
            const u32 rowbase = n1 + (u32)(srow >> kRowLog);
            if (P.f64) hoist_sp_row<ArF64>(P, A.tpr + ok * N + srow, A.logn1 == 0, rowbase, lane, lds, m, A.sp_fix, v);
            else hoist_sp_row<ArU64>(P, A.tpr + ok * N + srow, A.logn1 == 0, rowbase, lane, lds, m, A.sp_fix, v);
        }
        // the output positions this lane stores (layout C: four runs of four neighbours) and where each comes from in the source row
        u32 pl[kRowE];
        {
            const uint32_t *pb = pm + ((lane >> 2) << 6) + ((lane & 3) << 2);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint4 w = *reinterpret_cast<const uint4 *>(pb + (c << 4));
                pl[4 * c + 0] = (u32)lds_pad((int)hoist_src_elem(w.x)); pl[4 * c + 1] = (u32)lds_pad((int)hoist_src_elem(w.y));
                pl[4 * c + 2] = (u32)lds_pad((int)hoist_src_elem(w.z)); pl[4 * c + 3] = (u32)lds_pad((int)hoist_src_elem(w.w));
            }
        }
        lds_store_C(lds, lane, v);
        HE_WAVE_SYNC();
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = lds[pl[r]];
        u64 *arw = data ? A.aq + op * A.aq_op_stride + ((ok & 1) * (u64)A.L + (u64)idx) * N + arow : A.ap + ok * N + arow;
        if (A.first_a) {
#pragma unroll
            for (int r = 0; r < kRowE; ++r) acc[r] = 0;
        } else {
            load_rowC(arw, lane, acc);
        }
#pragma unroll
        for (int r = 0; r < kRowE; ++r) acc[r] = hoist_acc_term(acc[r], v[r], pt[r], m);
        store_rowC(arw, lane, acc);
        if (!data) return; // (wave-uniform: B lives under the data primes only)
        if (!poly0) {      // B[1] takes identity terms only: a keyed first term starts it at zero
            if (A.first_b) {
#pragma unroll
                for (int r = 0; r < kRowE; ++r) acc[r] = 0;
                store_rowC(A.out + ct_off + arow, lane, acc);
            }
            return;
        }
        load_rowC(A.in + ct_off + srow, lane, v); // c0's source row through the same permutation
        HE_WAVE_SYNC();                             // (every lane has read the key product's row out of LDS)
        lds_store_C(lds, lane, v);
        HE_WAVE_SYNC();
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = lds[pl[r]];
    }
    u64 *orow = A.out + ct_off + arow;
    if (A.first_b) {
#pragma unroll
        for (int r = 0; r < kRowE; ++r) acc[r] = 0;
    } else {
        load_rowC(orow, lane, acc);
    }
#pragma unroll
    for (int r = 0; r < kRowE; ++r) acc[r] = hoist_acc_term(acc[r], v[r], pt[r], m);
    store_rowC(orow, lane, acc);
}

struct PlainExtendArgs {
    const u64 *src;   // [n][L][N]: the plaintexts, NTT form (rows 0 .. L - 1 are copied)
    const u64 *coeff; // [n][Lc][N]: their rows 0 .. Lc - 1 in coefficient form; Lc = L with the check, else 1
    u64 *dst;         // [n][L + 1][N]: row L = the centred coefficients of row 0 mod P, coefficient form (the forward transform follows)
    u64 *mismatch;    // null: no check
    u64 n_polys;      // n (L + 1)
    int L, Lc, K, logN;
};
// streaming: a lane owns two neighbouring coefficients of one row of dst, 16-byte accesses
__global__ void __launch_bounds__(kBlock) k_plain_extend(PlainExtendArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1);
    if (p >= A.n_polys) return; // (a block lies inside one row: the whole block leaves)
    const u32 e2 = (u32)(gid & (((u64)1 << (A.logN - 1)) - 1));
    const int idx = (int)(p % (u64)(A.L + 1));
    const u64 item = p / (u64)(A.L + 1);
    ulonglong2 *d = reinterpret_cast<ulonglong2 *>(A.dst + (p << A.logN)) + e2;
    if (idx < A.L) *d = reinterpret_cast<const ulonglong2 *>(A.src + ((item * (u64)A.L + (u64)idx) << A.logN))[e2];
    if (idx == 0 || (idx < A.L && !A.mismatch)) return;
    const u64 q0 = primes[0].q, half0 = q0 >> 1;
    const ModU64 m = make_modu(primes[hoist_qp_prime(idx, A.L, A.K)]);
    const ulonglong2 c = reinterpret_cast<const ulonglong2 *>(A.coeff + ((item * (u64)A.Lc) << A.logN))[e2];
    const ulonglong2 w = make_ulonglong2(hoist_centred_mod(c.x, q0, half0, m), hoist_centred_mod(c.y, q0, half0, m));
    if (idx == A.L) {
        *d = w;
        return;
    }
    const ulonglong2 g = reinterpret_cast<const ulonglong2 *>(A.coeff + ((item * (u64)A.Lc + (u64)idx) << A.logN))[e2];
    const unsigned bad = (unsigned)__popcll(__ballot(g.x != w.x)) + (unsigned)__popcll(__ballot(g.y != w.y));
    if (bad && (threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long *>(A.mismatch), (unsigned long long)bad);
}

// ct [n_ops][2][L][N] -> dst, same layout: polynomial 0 copied, polynomial 1 zero
__global__ void __launch_bounds__(kBlock) k_hoist_addend_coeff(const u64 *ct, u64 *dst, int L, int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (logN - 1);
    if (p >= n_polys) return;
    const bool poly0 = ((p / (u64)L) & 1) == 0;
    reinterpret_cast<ulonglong2 *>(dst)[gid] = poly0 ? reinterpret_cast<const ulonglong2 *>(ct)[gid] : make_ulonglong2(0, 0);
}

// src [n_ops][2][L][N] = (c0 + u0, u1) -> out, same layout: coefficient o of every residue polynomial is +-src[gather[o]]
__global__ void __launch_bounds__(kBlock) k_hoist_finish_coeff(const u64 *src, u64 *out, const uint32_t *gather, const PrimeDev *primes, int L, int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (logN - 1);
    if (p >= n_polys) return;
    const u32 e2 = (u32)(gid & (((u64)1 << (logN - 1)) - 1));
    const u64 q = primes[(int)(p % (u64)L)].q;
    const uint2 g = reinterpret_cast<const uint2 *>(gather)[e2];
    const u64 *s = src + (p << logN);
    reinterpret_cast<ulonglong2 *>(out + (p << logN))[e2] =
        make_ulonglong2(hoist_gather_sign(s[hoist_gather_src(g.x)], g.x, q), hoist_gather_sign(s[hoist_gather_src(g.y)], g.y, q));
}

// ---- the baby-step/giant-step linear transform (he355_linear_transform_bsgs; arithmetic: bsgs_core.h) ----------------------------------
struct HoistRotArgs {
    const u64 *t;         // [n_ops][2][L][N]: one element's key product under the permuted key, data primes, canonical NTT form
    const u64 *tpr;       // [n_ops][2][N]: the same under the special prime after k_k3's inverse row pass (hoist_sp_row)
    const u64 *in;        // [n_ops][2][L][N]: the ciphertexts whose c1 was switched (c0 is read)
    const uint32_t *perm; // [N]: Params::galois_perm_ntt(g)
    u64 *dq;              // polynomial ok = op * 2 + k under data prime i: dq + ok * dq_poly_stride + i * N
    u64 dq_poly_stride;
    u64 *dp;              // ... under the special prime: dp + ok * dp_poly_stride
    u64 dp_poly_stride;
    u64 n_ops;
    int L, K, logn1;
    u64 sp_fix;           // as HoistAccArgs
};
// The sibling of k_hoist_acc_qp<true> without a plaintext: one wave per (ciphertext, polynomial, tile 0 .. L, row).  The key product's ONE
// source row -- plus P times the input's c0 row for polynomial 0 under a data prime, added BEFORE the permutation: both lie in the same
// source row, so one trip through the wave's LDS row carries both -- permuted and stored (!ACC: a baby term, or the first term of the giant
// accumulator) or added into what the destination holds (ACC: the giant step; one stream, launches in order).
template <bool ACC>
__global__ void __launch_bounds__(kBlock) k_hoist_rot_qp(HoistRotArgs A, const PrimeDev *primes)
{
    __shared__ u64 lds_all[kWaves][kLdsRow];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const int tiles = A.L + 1;
    const u64 total = (A.n_ops * 2 * (u64)tiles) << A.logn1;
    const u64 job = (u64)blockIdx.x * kWaves + wave;
    if (job >= total) return; // (the whole wave; waves of a block share nothing)
    const u32 a_row = (u32)(job & (n1 - 1));
    const u64 pi = job >> A.logn1; // (op, polynomial, tile)
    const int idx = (int)(pi % (u64)tiles);
    const u64 ok = pi / (u64)tiles; // op * 2 + polynomial
    const u64 N = (u64)n1 << kRowLog, arow = (u64)a_row << kRowLog;
    const PrimeDev &P = primes[hoist_qp_prime(idx, A.L, A.K)];
    const ModU64 m = make_modu(P);
    u64 *lds = lds_all[wave];
    const uint32_t *pm = A.perm + arow;
    const u64 srow = (u64)hoist_src_row(__builtin_amdgcn_readfirstlane(pm[0])) << kRowLog;
    const bool data = idx < A.L;
    u64 v[kRowE];
    if (data) {
        const u64 ct_off = (ok * (u64)A.L + (u64)idx) * N;
        load_rowC(A.t + ct_off + srow, lane, v);
        if ((ok & 1) == 0) { // (wave-uniform)
            const u64 pmq = bsgs_p_mod(primes[A.K - 1].q, m);
            u64 c[kRowE];
            load_rowC(A.in + ct_off + srow, lane, c);
#pragma unroll
            for (int r = 0; r < kRowE; ++r) v[r] = bsgs_fold_c0(v[r], c[r], pmq, m);
        }
    } else {
        const u32 rowbase = n1 + (u32)(srow >> kRowLog);
        if (P.f64) hoist_sp_row<ArF64>(P, A.tpr + ok * N + srow, A.logn1 == 0, rowbase, lane, lds, m, A.sp_fix, v);
        else hoist_sp_row<ArU64>(P, A.tpr + ok * N + srow, A.logn1 == 0, rowbase, lane, lds, m, A.sp_fix, v);
        HE_WAVE_SYNC(); // (the row pass is done with the LDS row)
    }
    // the output positions this lane stores (layout C: four runs of four neighbours) and where each comes from in the source row
    u32 pl[kRowE];
    {
        const uint32_t *pb = pm + ((lane >> 2) << 6) + ((lane & 3) << 2);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const uint4 w = *reinterpret_cast<const uint4 *>(pb + (c << 4));
            pl[4 * c + 0] = (u32)lds_pad((int)hoist_src_elem(w.x)); pl[4 * c + 1] = (u32)lds_pad((int)hoist_src_elem(w.y));
            pl[4 * c + 2] = (u32)lds_pad((int)hoist_src_elem(w.z)); pl[4 * c + 3] = (u32)lds_pad((int)hoist_src_elem(w.w));
        }
    }
    lds_store_C(lds, lane, v);
    HE_WAVE_SYNC();
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = lds[pl[r]];
    u64 *drow = (data ? A.dq + ok * A.dq_poly_stride + (u64)idx * N : A.dp + ok * A.dp_poly_stride) + arow;
    if constexpr (ACC) {
        u64 acc[kRowE];
        load_rowC(drow, lane, acc);
#pragma unroll
        for (int r = 0; r < kRowE; ++r) v[r] = bsgs_acc(acc[r], v[r], m.q);
    }
    store_rowC(drow, lane, v);
}

// The identity baby, streaming: dst [n_ops][2][L + 1][N] = (P c0, P c1) under the data primes and 0 under the special prime; a lane owns two
// neighbouring coefficients, 16-byte accesses
__global__ void __launch_bounds__(kBlock) k_bsgs_ident(const u64 *in, u64 *dst, const PrimeDev *primes, int L, int K, int logN, u64 n_polys)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (logN - 1); // (op, polynomial, tile)
    if (p >= n_polys) return;        // (a block lies inside one row: the whole block leaves)
    const u32 e2 = (u32)(gid & (((u64)1 << (logN - 1)) - 1));
    const int idx = (int)(p % (u64)(L + 1));
    const u64 ok = p / (u64)(L + 1);
    ulonglong2 w = make_ulonglong2(0, 0);
    if (idx < L) {
        const ModU64 m = make_modu(primes[idx]);
        const u64 pmq = bsgs_p_mod(primes[K - 1].q, m);
        const ulonglong2 c = reinterpret_cast<const ulonglong2 *>(in + ((ok * (u64)L + (u64)idx) << logN))[e2];
        w = make_ulonglong2(bsgs_ident_term(c.x, pmq, m), bsgs_ident_term(c.y, pmq, m));
    }
    reinterpret_cast<ulonglong2 *>(dst + (p << logN))[e2] = w;
}

struct BsgsInnerArgs {
    const u64 *store;     // [n_slots][n_ops][2][L + 1][N]: the baby terms
    const u64 *plain;     // the giant row's plaintexts, term i at plain + i * (L + 1) * N: [L + 1][N] each, shared by the chunk
    const uint2 *terms;   // [n_terms]: the row's used terms, (slot in the store, plaintext of the row)
    u32 n_terms;
    u64 run;              // bsgs_run: the terms one 128-bit sum takes
    u64 *dq;              // the sum's rows under the data primes, [n_ops][2][L][N] ...
    u64 *dp;              // ... and under the special prime, [n_ops][2][N]
    u64 n_ops;
    int L, K, logN;
    int acc;              // the identity row: the sum is added into what dq / dp hold (one load, one store)
};
// The inner sum of one giant row, streaming, no permutation: a lane owns two neighbouring coefficients of BOTH polynomials of one
// (ciphertext, tile) -- one pass over the row's used terms, the plaintext's 16 bytes loaded once per term for the two polynomials, four 128-bit
// sums, one reduction and one store each.  Blocks are numbered ciphertext-fastest: the blocks that are resident together read the SAME
// plaintext segments (once from HBM, then from L2 / the memory-side cache) and differ only in their own store rows.
__global__ void __launch_bounds__(kBlock) k_bsgs_inner(BsgsInnerArgs A, const PrimeDev *primes)
{
    const int seg_log = A.logN - 1 - 8; // blocks per row of N / 2 pairs (kBlock = 2^8 lanes)
    const u64 b = blockIdx.x;
    const u64 op = b % A.n_ops, rest = b / A.n_ops;
    const int idx = (int)(rest >> seg_log);
    if (idx > A.L) return; // (the whole block)
    const u64 e2 = ((rest & (((u64)1 << seg_log) - 1)) << 8) + threadIdx.x;
    const ModU64 m = make_modu(primes[hoist_qp_prime(idx, A.L, A.K)]);
    const u64 N = (u64)1 << A.logN, tile = (u64)(A.L + 1) * N;
    const u64 t_off = (op * 2 * (u64)(A.L + 1) + (u64)idx) * N, slot_stride = A.n_ops * 2 * tile;
    u128 s00 = 0, s01 = 0, s10 = 0, s11 = 0;
    u64 left = A.run;
    for (u32 k = 0; k < A.n_terms; ++k) {
        const uint2 tm = A.terms[k]; // (uniform)
        const ulonglong2 p = reinterpret_cast<const ulonglong2 *>(A.plain + (u64)tm.y * tile + (u64)idx * N)[e2];
        const u64 *t = A.store + (u64)tm.x * slot_stride + t_off;
        const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(t)[e2], c = reinterpret_cast<const ulonglong2 *>(t + tile)[e2];
        if (bsgs_run_full(left, A.run)) {
            bfv_mac_fold(s00, m); bfv_mac_fold(s01, m); bfv_mac_fold(s10, m); bfv_mac_fold(s11, m);
        }
        bfv_mac_add(s00, a.x, p.x); bfv_mac_add(s01, a.y, p.y); bfv_mac_add(s10, c.x, p.x); bfv_mac_add(s11, c.y, p.y);
        --left;
    }
    ulonglong2 r0 = make_ulonglong2(bfv_mac_reduce(s00, m), bfv_mac_reduce(s01, m)), r1 = make_ulonglong2(bfv_mac_reduce(s10, m), bfv_mac_reduce(s11, m));
    const bool data = idx < A.L;
    u64 *d0 = data ? A.dq + (op * 2 * (u64)A.L + (u64)idx) * N : A.dp + op * 2 * N;
    ulonglong2 *o0 = reinterpret_cast<ulonglong2 *>(d0) + e2, *o1 = reinterpret_cast<ulonglong2 *>(d0 + (data ? (u64)A.L * N : N)) + e2;
    if (A.acc) {
        const ulonglong2 x = *o0, y = *o1;
        r0 = make_ulonglong2(bsgs_acc(x.x, r0.x, m.q), bsgs_acc(x.y, r0.y, m.q));
        r1 = make_ulonglong2(bsgs_acc(y.x, r1.x, m.q), bsgs_acc(y.y, r1.y, m.q));
    }
    *o0 = r0;
    *o1 = r1;
}

} // namespace

void launch_hoist_rot_qp(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *tpr, const u64 *in, const uint32_t *perm, u64 *dq, u64 dq_poly_stride, u64 *dp,
                         u64 dp_poly_stride, bool acc)
{
    if (!n_ops) return;
    if (!t || !tpr || !in || !perm || !dq || !dp) throw std::runtime_error("linear transform: the rotate kernel needs both halves of the key product, the input, the permutation and the destination");
    HoistRotArgs A{};
    A.t = t; A.tpr = tpr; A.in = in; A.perm = perm; A.dq = dq; A.dq_poly_stride = dq_poly_stride; A.dp = dp; A.dp_poly_stride = dp_poly_stride;
    A.n_ops = n_ops; A.L = L; A.K = env.K; A.logn1 = env.logn1;
    A.sp_fix = env.logn1 ? hoist_row_pass_fix(env.prime_q[env.K - 1]) : 1;
    const u64 jobs = (n_ops * 2 * (u64)(L + 1)) << env.logn1;
    const dim3 g(grid_blocks((jobs + kWaves - 1) / kWaves, "linear transform", "ciphertexts"));
    if (acc) hipLaunchKernelGGL(k_hoist_rot_qp<true>, g, dim3(kBlock), 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL(k_hoist_rot_qp<false>, g, dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bsgs_ident(const KernelEnv &env, int L, u64 n_ops, const u64 *in, u64 *dst)
{
    if (!n_ops) return;
    const int logN = env.logn1 + kRowLog;
    const u64 n_polys = n_ops * 2 * (u64)(L + 1);
    hipLaunchKernelGGL(k_bsgs_ident, dim3(streaming_grid(n_polys, logN, "linear transform", "ciphertexts")), dim3(kBlock), 0, env.stream, in, dst, env.primes, L, env.K, logN,
                       n_polys);
}
void launch_bsgs_inner(const KernelEnv &env, int L, u64 n_ops, const u64 *store, const u64 *plain_row, const uint32_t *terms, u64 n_terms, u64 *dq, u64 *dp, bool acc)
{
    if (!n_ops) return;
    if (!n_terms || n_terms > 0xffffffffull) throw std::runtime_error("linear transform: an inner sum takes between one and 2^32 - 1 terms");
    BsgsInnerArgs A{};
    A.store = store; A.plain = plain_row; A.terms = reinterpret_cast<const uint2 *>(terms); A.n_terms = (u32)n_terms;
    u64 q[kMaxPrimes];
    for (int i = 0; i <= L; ++i) q[i] = env.prime_q[hoist_qp_prime(i, L, env.K)];
    A.run = bsgs_run(q, L + 1);
    A.dq = dq; A.dp = dp; A.n_ops = n_ops; A.L = L; A.K = env.K; A.logN = env.logn1 + kRowLog; A.acc = acc ? 1 : 0;
    const u64 blocks = (n_ops * (u64)(L + 1)) << (A.logN - 9);
    hipLaunchKernelGGL(k_bsgs_inner, dim3(grid_blocks(blocks, "linear transform", "ciphertexts")), dim3(kBlock), 0, env.stream, A, env.primes);
}

void launch_key_permute(const KernelEnv &env, const u64 *src, u64 *dst, const uint32_t *perm, u64 n_polys)
{
    if (!n_polys) return;
    const int logN = env.logn1 + kRowLog;
    hipLaunchKernelGGL(k_key_permute, dim3(streaming_grid(n_polys, logN, "hoisted rotation")), dim3(kBlock), 0, env.stream, src, dst, perm, logN, n_polys);
}
void launch_hoist_finish_ntt(const KernelEnv &env, int L, u64 n_ops, const u64 *u, const u64 *in, const uint32_t *perm, u64 *out, const u64 *plain, bool first)
{
    if (!n_ops) return;
    HoistNttArgs A{};
    A.u = u; A.in = in; A.perm = perm; A.out = out; A.plain = plain; A.n_ops = n_ops; A.L = L; A.logn1 = env.logn1; A.first = first ? 1 : 0;
    const u64 jobs = (n_ops * 2 * (u64)L) << env.logn1;
    const dim3 g(grid_blocks((jobs + kWaves - 1) / kWaves, "hoisted rotation", "ciphertexts"));
    if (plain) hipLaunchKernelGGL(k_hoist_finish_ntt<true>, g, dim3(kBlock), 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL(k_hoist_finish_ntt<false>, g, dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_hoist_acc_qp(const KernelEnv &env, int L, u64 n_ops, const u64 *t, const u64 *tpr, const u64 *in, const uint32_t *perm, const u64 *plain_qp, u64 *aq,
                         u64 aq_op_stride, u64 *ap, u64 *out, bool first_a, bool first_b)
{
    if (!n_ops) return;
    const bool keyed = t != nullptr;
    if (keyed && (!tpr || !perm || !aq || !ap)) throw std::runtime_error("lazy plain sum: a keyed term needs both halves of the key product, the permutation and the accumulators");
    HoistAccArgs A{};
    A.t = t; A.tpr = tpr; A.in = in; A.perm = perm; A.plain = plain_qp; A.aq = aq; A.aq_op_stride = aq_op_stride; A.ap = ap; A.out = out;
    A.n_ops = n_ops; A.L = L; A.K = env.K; A.logn1 = env.logn1;
    A.sp_fix = env.logn1 ? hoist_row_pass_fix(env.prime_q[env.K - 1]) : 1;
    A.first_a = first_a ? 1 : 0; A.first_b = first_b ? 1 : 0;
    const u64 jobs = (n_ops * 2 * (u64)(keyed ? L + 1 : L)) << env.logn1;
    const dim3 g(grid_blocks((jobs + kWaves - 1) / kWaves, "lazy plain sum", "ciphertexts"));
    if (keyed) hipLaunchKernelGGL(k_hoist_acc_qp<true>, g, dim3(kBlock), 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL(k_hoist_acc_qp<false>, g, dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_plain_extend(const KernelEnv &env, int L, u64 n, const u64 *src, const u64 *coeff, int Lc, u64 *dst, u64 *mismatch)
{
    if (!n) return;
    if (Lc != (mismatch ? L : 1)) throw std::runtime_error("plaintext extension: the coefficient rows are row 0 alone, or all rows with the check");
    PlainExtendArgs A{};
    A.src = src; A.coeff = coeff; A.dst = dst; A.mismatch = mismatch; A.n_polys = n * (u64)(L + 1); A.L = L; A.Lc = Lc; A.K = env.K;
    A.logN = env.logn1 + kRowLog;
    hipLaunchKernelGGL(k_plain_extend, dim3(streaming_grid(A.n_polys, A.logN, "plaintext extension", "plaintexts")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_hoist_addend_coeff(const KernelEnv &env, int L, u64 n_ops, const u64 *ct, u64 *dst)
{
    if (!n_ops) return;
    const int logN = env.logn1 + kRowLog;
    const u64 n_polys = n_ops * 2 * (u64)L;
    hipLaunchKernelGGL(k_hoist_addend_coeff, dim3(streaming_grid(n_polys, logN, "hoisted rotation", "ciphertexts")), dim3(kBlock), 0, env.stream, ct, dst, L, logN, n_polys);
}
void launch_hoist_finish_coeff(const KernelEnv &env, int L, u64 n_ops, const u64 *src, const uint32_t *gather, u64 *out)
{
    if (!n_ops) return;
    const int logN = env.logn1 + kRowLog;
    const u64 n_polys = n_ops * 2 * (u64)L;
    hipLaunchKernelGGL(k_hoist_finish_coeff, dim3(streaming_grid(n_polys, logN, "hoisted rotation", "ciphertexts")), dim3(kBlock), 0, env.stream, src, out, gather, env.primes, L,
                       logN, n_polys);
}

} // namespace HE355_KNS
} // namespace he355
