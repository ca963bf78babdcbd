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
//   k_hoist_addend_coeff   streaming, once per chunk (BFV coefficient form): (c0, 0), what launch_bfv_tail_fin adds every element's key
//                          switch into.
//   k_hoist_finish_coeff   streaming: the signed gather of Params::galois_gather_coeff(g) on (c0 + u0, u1); a lane gathers two coefficients
//                          and makes one 16-byte store.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

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

} // namespace

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
