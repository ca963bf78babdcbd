// he355_kernels_bfv_noise.hip -- the BFV invariant noise budget (Decryptor::invariant_noise_budget) of a batch of coefficient-form
// ciphertexts.  The per-coefficient arithmetic is bfv_noise_core.h (host-compilable: tests/csim_bfv_noise and the host client run the
// same text on the CPU); the transforms around these kernels are the generic launch_ntt_forward / launch_ntt_inverse.
//
//   k_bfv_noise_take     streaming; copies polynomials 1 .. size-1 of every ciphertext of a chunk into scratch for the forward transform
//                        (polynomial 0 is never transformed: it is added in coefficient form by k_bfv_noise_bits).
//   k_bfv_noise_dot_sk   NTT form, (c_{size-1} s + .. + c_1) s per prime: Horner in s without the constant term.
//   k_bfv_noise_bits<W>  one thread per coefficient over the whole chunk: bfv_noise_bits<W> in registers (c0 added, times t, CRT-composed,
//                        centred, bit length), maximum over the wave by __shfl_xor, over the block through LDS, ONE atomicMax per block
//                        into the ciphertext's word (N / 256 atomics per ciphertext on one address: 4 at N = 1024, 128 at N = 32768).
//   k_bfv_noise_finish   budget = max(0, bits(q_L) - noise_bits - 1) per ciphertext, in place on the word the maxima were gathered in (the
//                        caller's d_budget, zeroed by hipMemsetAsync on the same stream: no scratch word, one launch per call).
#include <hip/hip_runtime.h>

#include <stdexcept>

#include "he355_kernels.h"
#include "bfv_noise_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_noise.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;
// a block of k_bfv_noise_bits never straddles two ciphertexts: N is a power of two >= 1024 (he_params.cpp), a multiple of kBlock
static_assert(1024 % kBlock == 0 && kBlock % kWave == 0, "a block lies inside one polynomial and is whole waves");

inline unsigned grid_for(u64 jobs, u64 per_block) { return (unsigned)((jobs + per_block - 1) / per_block); }

// ct [.][size][L][N] -> tmp [n_cts][size - 1][L][N]; one thread = 2 coefficients
__global__ void __launch_bounds__(kBlock) k_bfv_noise_take(const u64 *ct, u64 *tmp, int L, int size, int logN, u64 n_cts)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 pp = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    const u64 per = (u64)(size - 1) * L, r = pp / per;
    if (r >= n_cts) return;
    const u64 p = pp - r * per;
    reinterpret_cast<ulonglong2 *>(tmp + ((r * per + p) << logN))[e2] = reinterpret_cast<const ulonglong2 *>(ct + ((r * size * L + L + p) << logN))[e2];
}
// tmp [n_cts][size - 1][L][N] NTT form (c_1 .. c_{size-1}), sk [K][N] -> out [n_cts][L][N] = (c_{size-1} s + .. + c_1) s
__global__ void __launch_bounds__(kBlock) k_bfv_noise_dot_sk(const u64 *tmp, const u64 *sk, u64 *out, const PrimeDev *primes, int L, int size, int logN, u64 n_cts)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 pp = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    const u64 r = pp / L;
    if (r >= n_cts) return;
    const int i = (int)(pp % L), np = size - 1;
    const PrimeDev &P = primes[i];
    const ModU64 m = bfv_modu(P);
    const ulonglong2 s = reinterpret_cast<const ulonglong2 *>(sk + ((u64)i << logN))[e2];
    ulonglong2 acc = reinterpret_cast<const ulonglong2 *>(tmp + (((r * np + np - 1) * L + i) << logN))[e2];
    for (int k = np - 2; k >= 0; --k) {
        const ulonglong2 c = reinterpret_cast<const ulonglong2 *>(tmp + (((r * np + k) * L + i) << logN))[e2];
        acc.x = addmod(barrett128((u128)acc.x * s.x, m), c.x, P.q);
        acc.y = addmod(barrett128((u128)acc.y * s.y, m), c.y, P.q);
    }
    acc.x = barrett128((u128)acc.x * s.x, m);
    acc.y = barrett128((u128)acc.y * s.y, m);
    reinterpret_cast<ulonglong2 *>(out + ((r * L + i) << logN))[e2] = acc;
}
// part [n_cts][L][N] coefficient form (the key-dependent part of the phase), ct [.][size][L][N] (polynomial 0 is read) -> bits [n_cts],
// zeroed by the caller on the same stream
template <int W>
__global__ void __launch_bounds__(kBlock) k_bfv_noise_bits(const u64 *part, const u64 *ct, int *bits, const PrimeDev *primes, BfvNoiseConst c, BfvNoiseView v, int size,
                                                           int logN, u64 n_cts)
{
    constexpr int L = W - 2;
    __shared__ int wave_max[kBlock / kWave];
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 r = gid >> logN, n = gid & (((u64)1 << logN) - 1);
    if (r >= n_cts) return; // the whole block: it lies inside one ciphertext
    int b = bfv_noise_bits<W>(part + ((r * L) << logN) + n, ct + ((r * size * L) << logN) + n, (u64)1 << logN, primes, c, v);
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) b = max(b, __shfl_xor(b, o, kWave));
    if ((threadIdx.x & (kWave - 1)) == 0) wave_max[threadIdx.x / kWave] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / kWave; ++w) b = max(b, wave_max[w]);
        atomicMax(bits + r, b);
    }
}
// budget [n_cts]: noise bits in, budget out
__global__ void __launch_bounds__(kBlock) k_bfv_noise_finish(int *budget, int *noise_bits, int q_bits, u64 n_cts)
{
    const u64 r = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_cts) return;
    const int nb = budget[r];
    budget[r] = bfv_noise_budget_of(q_bits, nb);
    if (noise_bits) noise_bits[r] = nb;
}

} // namespace

void launch_bfv_noise_take(const KernelEnv &env, int L, int size, u64 n_cts, const u64 *ct, u64 *tmp)
{
    if (!n_cts || size < 2) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_cts * (u64)(size - 1) * L) << (logN - 1);
    hipLaunchKernelGGL(k_bfv_noise_take, dim3(grid_for(threads, kBlock)), dim3(kBlock), 0, env.stream, ct, tmp, L, size, logN, n_cts);
}
void launch_bfv_noise_dot_sk(const KernelEnv &env, int L, int size, u64 n_cts, const u64 *tmp, const u64 *sk, u64 *out)
{
    if (!n_cts) return;
    const int logN = env.logn1 + kRowLog;
    const u64 threads = (n_cts * L) << (logN - 1);
    hipLaunchKernelGGL(k_bfv_noise_dot_sk, dim3(grid_for(threads, kBlock)), dim3(kBlock), 0, env.stream, tmp, sk, out, env.primes, L, size, logN, n_cts);
}
void launch_bfv_noise_bits(const KernelEnv &env, int size, u64 n_cts, const u64 *part, const u64 *ct, int *bits, const CrtTablesDev &crt, const BfvNoiseConst &c)
{
    if (!n_cts) return;
    const int logN = env.logn1 + kRowLog;
    const unsigned grid = grid_for(n_cts << logN, kBlock);
    BfvNoiseView v;
    v.Q = crt.Q; v.halfQ = crt.halfQ; v.punct = crt.punct;
#define HE355_NOISE(W) case W: hipLaunchKernelGGL(k_bfv_noise_bits<W>, dim3(grid), dim3(kBlock), 0, env.stream, part, ct, bits, env.primes, c, v, size, logN, n_cts); break;
    switch (crt.words) { // words = L + 2 (DeviceContext::crt_tables), L <= 16
        HE355_NOISE(3) HE355_NOISE(4) HE355_NOISE(5) HE355_NOISE(6) HE355_NOISE(7) HE355_NOISE(8) HE355_NOISE(9) HE355_NOISE(10)
        HE355_NOISE(11) HE355_NOISE(12) HE355_NOISE(13) HE355_NOISE(14) HE355_NOISE(15) HE355_NOISE(16) HE355_NOISE(17) HE355_NOISE(18)
    default: throw std::invalid_argument("launch_bfv_noise_bits: CRT tables of 1 to 16 data primes");
    }
#undef HE355_NOISE
}
void launch_bfv_noise_finish(const KernelEnv &env, u64 n_cts, int *budget, int *noise_bits, int q_bits)
{
    if (!n_cts) return;
    hipLaunchKernelGGL(k_bfv_noise_finish, dim3(grid_for(n_cts, kBlock)), dim3(kBlock), 0, env.stream, budget, noise_bits, q_bits, n_cts);
}

} // namespace HE355_KNS
} // namespace he355
