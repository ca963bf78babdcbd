// he355_kernels_bfv_reply.hip -- BFV reply compression: an L = 1 ciphertext switched to the moduli 2^k0 / 2^k1 and bit-packed
// (he355_bfv_reply_compress), and the client's decryption of such replies (he355_bfv_reply_decrypt).  The arithmetic is bfv_reply_core.h
// (host-compilable: tests/csim/sim_bfv_reply.cpp runs the same text on the CPU); the transforms and the product with the secret key between
// k_bfv_reply_lift and k_bfv_reply_finish are the generic launch_ntt_forward / launch_bfv_noise_dot_sk / launch_ntt_inverse at prime 0.
//
//   k_bfv_reply_pack     streaming; a lane owns ONE output word of one reply: it switches the coefficients that touch the word
//                        (64 / k + 2 at the most) and makes one 8-byte store.  A coefficient whose field straddles two words is switched by
//                        both owners -- one high and one low product and two compares, against the 8-byte load its neighbour lane
//                        already brought into the cache -- so nothing is staged through LDS and no lane waits on another.  No atomics,
//                        no partial stores.  A block owns 256 neighbouring words of one reply: c0's N k0 / 64 words, then c1's N k1 / 64.
//   k_bfv_reply_lift     streaming; a lane owns two neighbouring coefficients of c1: cut out of the reply's words, centred, lifted mod q_0,
//                        one 16-byte store into client scratch.
//   k_bfv_reply_finish   one lane per coefficient: c0's field, plus the centred product, rounded to the plaintext coefficient; the bit
//                        length of the residue is reduced over the wave by __shfl_xor, over the block through LDS, ONE atomicMax per block
//                        into the reply's word (as k_bfv_noise_bits).  NEED_BITS false (both outputs NULL): no reduction at all.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "bfv_reply_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_reply.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

constexpr int kWave = 64;
static_assert(1024 % kBlock == 0 && kBlock % kWave == 0, "a block of k_bfv_reply_finish lies inside one reply and is whole waves");

// reply j: the words at bytes + j stride, c0's N k0 / 64 then c1's N k1 / 64
struct BfvReplyArgs {
    const unsigned char *bytes_in; // decrypt: the replies
    unsigned char *bytes_out;      // compress: the target
    const u64 *ct;                 // compress: [n][2][N], L = 1, coefficient form
    u64 n, stride, t, q;
    u32 w0, w1; // words of the two halves
    u32 bpr;    // compress: blocks per reply, ceil((w0 + w1) / kBlock)
    int k0, k1, logN;
    BfvReplyCut cut0, cut1; // compress: the switch of each half
};

__global__ void __launch_bounds__(kBlock) k_bfv_reply_pack(BfvReplyArgs A)
{
    // neighbouring blocks own neighbouring words of ONE reply: the blocks in flight read a contiguous stretch of the ciphertext slab instead
    // of the same offset of many replies, which lie a power of two apart
    const u32 j = blockIdx.x / A.bpr;
    const u32 g = (blockIdx.x - j * A.bpr) * kBlock + threadIdx.x;
    if (g >= A.w0 + A.w1) return;
    const bool second = g >= A.w0;
    const u64 *coef = A.ct + ((((u64)j << 1) | (second ? 1 : 0)) << A.logN);
    reinterpret_cast<u64 *>(A.bytes_out + (u64)j * A.stride)[g] = bfv_reply_pack_word(coef, second ? g - A.w0 : g, second ? A.cut1 : A.cut0);
}

// -> out [n][N]: c1 centred and lifted mod q_0
__global__ void __launch_bounds__(kBlock) k_bfv_reply_lift(BfvReplyArgs A, u64 *out)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 j = gid >> (A.logN - 1);
    const u32 e2 = (u32)(gid & (((u64)1 << (A.logN - 1)) - 1));
    if (j >= A.n) return;
    const u64 *w = reinterpret_cast<const u64 *>(A.bytes_in + j * A.stride) + A.w0;
    const u64 q = A.q;
    reinterpret_cast<ulonglong2 *>(out + (j << A.logN))[e2] =
        make_ulonglong2(bfv_reply_lift(bfv_reply_field(w, 2 * e2, A.k1), A.k1, q), bfv_reply_lift(bfv_reply_field(w, 2 * e2 + 1, A.k1), A.k1, q));
}

// prod [n][N] (the product's residues mod q_0) -> plain [n][N]; bits [n], zeroed by the caller on the same stream
template <bool NEED_BITS>
__global__ void __launch_bounds__(kBlock) k_bfv_reply_finish(BfvReplyArgs A, const u64 *prod, u64 *plain, int *bits)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 j = gid >> A.logN;
    const u32 e = (u32)(gid & (((u64)1 << A.logN) - 1));
    if (j >= A.n) return; // the whole block: it lies inside one reply
    const u64 y0 = bfv_reply_field(reinterpret_cast<const u64 *>(A.bytes_in + j * A.stride), e, A.k0);
    const BfvReplyCoef c = bfv_reply_round(y0, prod[gid], A.k0, A.k1, A.q, A.t);
    plain[gid] = c.m;
    if constexpr (NEED_BITS) {
        __shared__ int wave_max[kBlock / kWave];
        int b = c.bits;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) b = max(b, __shfl_xor(b, o, kWave));
        if ((threadIdx.x & (kWave - 1)) == 0) wave_max[threadIdx.x / kWave] = b;
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 1; w < kBlock / kWave; ++w) b = max(b, wave_max[w]);
            atomicMax(bits + j, b);
        }
    }
}

BfvReplyArgs reply_args(const KernelEnv &env, int k0, int k1, u64 n, u64 stride)
{
    const u64 N = (u64)1 << (env.logn1 + kRowLog), q = env.prime_q[0];
    if (!bfv_reply_widths_ok(N, q, k0, k1) || (stride & 7) || stride < bfv_reply_size(N, k0, k1))
        throw std::invalid_argument("reply compression: widths or stride out of range");
    BfvReplyArgs A{};
    A.n = n; A.stride = stride; A.q = q; A.k0 = k0; A.k1 = k1; A.logN = env.logn1 + kRowLog;
    A.w0 = (u32)bfv_reply_half_words(N, k0); A.w1 = (u32)bfv_reply_half_words(N, k1);
    return A;
}
void need_aligned(const void *bytes)
{
    if ((unsigned long long)bytes & 7) throw std::invalid_argument("reply compression: the replies must be 8-byte aligned");
}
unsigned coef_grid(u64 n, int logN) { return grid_blocks((n << logN) / kBlock, "reply compression", "replies"); }

} // namespace

void launch_bfv_reply_pack(const KernelEnv &env, int k0, int k1, u64 n, const u64 *ct, u64 stride, void *bytes)
{
    if (!n) return;
    BfvReplyArgs A = reply_args(env, k0, k1, n, stride);
    need_aligned(bytes);
    A.ct = ct; A.bytes_out = static_cast<unsigned char *>(bytes); A.cut0 = bfv_reply_cut_of(A.q, k0); A.cut1 = bfv_reply_cut_of(A.q, k1);
    A.bpr = (A.w0 + A.w1 + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_bfv_reply_pack, dim3(grid_blocks(n * A.bpr, "reply compression", "replies")), dim3(kBlock), 0, env.stream, A);
}
void launch_bfv_reply_lift(const KernelEnv &env, int k0, int k1, u64 n, const void *bytes, u64 stride, u64 *out)
{
    if (!n) return;
    BfvReplyArgs A = reply_args(env, k0, k1, n, stride);
    need_aligned(bytes);
    A.bytes_in = static_cast<const unsigned char *>(bytes);
    hipLaunchKernelGGL(k_bfv_reply_lift, dim3(streaming_grid(n, A.logN, "reply compression", "replies")), dim3(kBlock), 0, env.stream, A, out);
}
void launch_bfv_reply_finish(const KernelEnv &env, int k0, int k1, u64 t, u64 n, const void *bytes, u64 stride, const u64 *prod, u64 *plain, int *bits)
{
    if (!n) return;
    BfvReplyArgs A = reply_args(env, k0, k1, n, stride);
    need_aligned(bytes);
    A.bytes_in = static_cast<const unsigned char *>(bytes); A.t = t;
    const dim3 g(coef_grid(n, A.logN)), b(kBlock);
    if (bits) hipLaunchKernelGGL(k_bfv_reply_finish<true>, g, b, 0, env.stream, A, prod, plain, bits);
    else hipLaunchKernelGGL(k_bfv_reply_finish<false>, g, b, 0, env.stream, A, prod, plain, bits);
}

} // namespace HE355_KNS
} // namespace he355
