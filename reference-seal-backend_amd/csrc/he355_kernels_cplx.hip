// he355_kernels_cplx.hip -- complex CKKS slots on the device: the complex scalar combination (he355_combine_scalars_complex; the leaves of
// he355_ckks_eval_poly_complex) and the complex ends of the codec (he355_ckks_encode_complex, he355_ckks_decode_complex).  The
// per-coefficient arithmetic of the combination is cplx_core.h (host-compilable: tests/csim/sim_cplx.cpp runs the same text on the CPU);
// the floating-point work of the codec is client/ckks_codec.h's, shared with the host client.
//
//   k_scalar_combine_cplx  k_scalar_combine's lane program (he355_kernels_poly.hip) with the scalar and the opening constant picked by
//                          s(e) = bit (log2 N - 2) of the NTT index: the tables hold two residues per (term, prime), [n_terms][2][L] and
//                          [2][L].  A wave owns 128 neighbouring coefficients and N / 4 >= 256, so s is wave-uniform (read through
//                          readfirstlane: the scalar stays one uniform load per term).  Streaming, 16-byte accesses, one store, no LDS.
//   k_ckks_encode_cplx     k_ckks_encode with z[slot] = v and z[conjugate slot] = conj(v); everything behind the placement is the same text.
//   k_ckks_gather_cplx     the (re, im) pairs of the wanted slots out of the transform k_ckks_decode_fft left in its buffer.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "he355_kernels.h"
#include "cplx_core.h"
#include "ntt_core.h"
#include "client/ckks_codec.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_cplx.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

struct ScalarCombineCplxArgs {
    const ulonglong2 *terms; // [n_terms]: {the term's slab, its level L_t}
    const u64 *scalars;      // [n_terms][2][L]
    const u64 *cst;          // [2][L], or null: no constant
    u64 *out;                // [n][size][L][N]
    u64 n;
    u64 run;                 // poly_run
    u32 n_terms;
    int L, size, logN;
};

__global__ void __launch_bounds__(kBlock) k_scalar_combine_cplx(ScalarCombineCplxArgs A, const PrimeDev *primes)
{
    const int seg_log = A.logN - 1 - 8; // blocks per row of N / 2 pairs (kBlock = 2^8 lanes)
    const u64 b = blockIdx.x;
    const u64 c = b % A.n, rest = b / A.n;
    const u64 pi = rest >> seg_log; // (polynomial, prime)
    const int i = (int)(pi % (u64)A.L), k = (int)(pi / (u64)A.L);
    if (k >= A.size) return; // (the whole block; the grid is exact)
    const u64 e2 = ((rest & (((u64)1 << seg_log) - 1)) << 8) + threadIdx.x;
    const u32 s = (u32)__builtin_amdgcn_readfirstlane((int)cplx_half(2 * e2, A.logN)); // (both coefficients of the pair, all lanes of the wave)
    const ModU64 m = make_modu(primes[i]);
    const u64 N = (u64)1 << A.logN;
    const u64 ck = c * (u64)A.size + (u64)k;
    const u64 *sc = A.scalars + (u64)s * (u64)A.L + (u64)i;
    u128 s0 = (k == 0 && A.cst) ? A.cst[(u64)s * (u64)A.L + (u64)i] : 0, s1 = s0;
    u64 left = A.run - 1;
#pragma unroll 2
    for (u32 t = 0; t < A.n_terms; ++t) {
        const ulonglong2 tm = A.terms[t]; // (uniform)
        const u64 a = sc[(u64)t * 2 * (u64)A.L];
        const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(reinterpret_cast<const u64 *>(tm.x) + (ck * tm.y + (u64)i) * N)[e2];
        if (bsgs_run_full(left, A.run)) {
            bfv_mac_fold(s0, m); bfv_mac_fold(s1, m);
        }
        bfv_mac_add(s0, x.x, a); bfv_mac_add(s1, x.y, a);
        --left;
    }
    reinterpret_cast<ulonglong2 *>(A.out + (ck * (u64)A.L + (u64)i) * N)[e2] = make_ulonglong2(bfv_mac_reduce(s0, m), bfv_mac_reduce(s1, m));
}

// ---- the complex ends of the codec (one 1024-thread workgroup per vector, as k_ckks_encode / k_ckks_decode_fft) ----------------------
constexpr int kEncBlock = 1024;
// values [n][count][2] doubles (re, im) -> plain [n][Ltop][N] integer coefficients as residues (coefficient form; the caller transforms them)
__global__ void __launch_bounds__(kEncBlock) k_ckks_encode_cplx(const double *values, u64 count, double scale, client::Cplx *zbuf, u64 *plain,
                                                                const uint32_t *slot_index, const client::Cplx *W, const client::Cplx *Z, const PrimeDev *primes,
                                                                int Ltop, int logN, int *err)
{
    const u32 N = 1u << logN, half = N >> 1;
    const u64 r = blockIdx.x;
    client::Cplx *z = zbuf + r * N;
    for (u32 n = threadIdx.x; n < N; n += kEncBlock) z[n] = client::Cplx{0.0, 0.0};
    __syncthreads();
    for (u32 i = threadIdx.x; i < count; i += kEncBlock) {
        const client::Cplx v{values[(r * count + i) * 2], values[(r * count + i) * 2 + 1]};
        z[client::bitrev_u32(slot_index[i], logN)] = v;
        z[client::bitrev_u32(slot_index[half + i], logN)] = client::cconj(v);
    }
    __syncthreads();
    for (u32 len = 2; len <= N; len <<= 1) {
        for (u32 t = threadIdx.x; t < N / 2; t += kEncBlock) client::fft_stage_bfly(z, W, len, t, false);
        __syncthreads();
    }
    for (u32 n = threadIdx.x; n < N; n += kEncBlock) {
        const double rv = client::ckks_encode_coeff(z[n], Z[n], (double)N, scale);
        long long iv = 0;
        if (!(fabs(rv) < 9.2e18)) atomicOr(err, 1);
        else iv = (long long)rv;
        for (int i = 0; i < Ltop; ++i) {
            const u64 q = primes[i].q;
            const u64 m = iv >= 0 ? (u64)iv % q : (u64)(-iv) % q;
            plain[((r * Ltop + i) << logN) + n] = (iv >= 0 || m == 0) ? m : q - m;
        }
    }
}
// one thread per wanted slot: gid = r * sr.total + position inside the concatenated ranges; zbuf holds the finished transforms
__global__ void __launch_bounds__(kBlock) k_ckks_gather_cplx(const client::Cplx *zbuf, client::Cplx *out, const uint32_t *slot_index, int logN, u64 n_vec, SlotRanges sr)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 r = gid / sr.total;
    if (r >= n_vec) return;
    u32 pos = (u32)(gid - r * sr.total), g = 0;
    while (pos >= sr.count[g]) pos -= sr.count[g++];
    out[gid] = zbuf[(r << logN) + slot_index[sr.first[g] + pos]];
}

} // namespace

void launch_scalar_combine_cplx(const KernelEnv &env, int L, int size, u64 n, const void *d_terms, u64 n_terms, const u64 *d_scalars, const u64 *d_const, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || size < 1 || size > 3 || !n_terms || n_terms > 0xffffffffull || !d_terms || !d_scalars || !out)
        throw std::runtime_error("he355_combine_scalars_complex: the launch needs a level, a size of 1..3, between one and 2^32 - 1 terms and its tables");
    ScalarCombineCplxArgs A{};
    A.terms = reinterpret_cast<const ulonglong2 *>(d_terms); A.scalars = d_scalars; A.cst = d_const; A.out = out;
    A.n = n; A.n_terms = (u32)n_terms; A.L = L; A.size = size; A.logN = env.logn1 + kRowLog;
    A.run = poly_run(env.prime_q, L);
    if (A.run < 2) throw std::runtime_error("he355_combine_scalars_complex: prime too wide for a 128-bit sum");
    const u64 blocks = (n * (u64)size * (u64)L) << (A.logN - 9);
    hipLaunchKernelGGL(k_scalar_combine_cplx, dim3(grid_blocks(blocks, "he355_combine_scalars_complex", "ciphertexts")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_ckks_encode_cplx(const KernelEnv &env, u64 n_vec, const double *values, u64 count, double scale, void *zbuf, u64 *plain, const EncTablesDev &t, int *err)
{
    if (!n_vec) return;
    hipLaunchKernelGGL(k_ckks_encode_cplx, dim3((unsigned)n_vec), dim3(kEncBlock), 0, env.stream, values, count, scale, static_cast<client::Cplx *>(zbuf), plain,
                       t.slot_index, static_cast<const client::Cplx *>(t.W), static_cast<const client::Cplx *>(t.Z), env.primes, env.Ltop, env.logn1 + kRowLog, err);
}
void launch_ckks_gather_cplx(const KernelEnv &env, u64 n_vec, const void *zbuf, double *out, const EncTablesDev &t, const SlotRanges &sr)
{
    if (!n_vec || !sr.total) return;
    const u64 jobs = n_vec * sr.total;
    hipLaunchKernelGGL(k_ckks_gather_cplx, dim3((unsigned)((jobs + kBlock - 1) / kBlock)), dim3(kBlock), 0, env.stream, static_cast<const client::Cplx *>(zbuf),
                       reinterpret_cast<client::Cplx *>(out), t.slot_index, env.logn1 + kRowLog, n_vec, sr);
}

} // namespace HE355_KNS
} // namespace he355
