// he355_kernels_bfv_bytes.hip -- a PIR database from packed bytes to BFV plaintexts and back: he355_bfv_unpack_bytes,
// he355_bfv_unpack_bytes_ntt, he355_bfv_pack_bytes.  The arithmetic is bfv_bytes_core.h (host-compilable: tests/csim/sim_bfv_bytes.cpp and
// tests/bfv_bytes_guard_main.cpp run the same text on the CPU) and bfv_level_core.h's centred lift.
//
//   k_bfv_unpack         streaming; a lane owns two neighbouring coefficients of one plaintext: at most two aligned 8-byte loads per
//                        coefficient (the lanes of a wave share them: w bits apart), one 16-byte store.
//   k_bfv_pack           the inverse; a lane owns ONE output word of one plaintext: it ORs in the coefficients that touch the word
//                        (64 / w + 2 at the most) and makes one 8-byte store.  No atomics, no partial-byte stores.  The grid is (plaintext, 256 words).
//   k_bfv_bytes_cols_fwd<LOGN1>   he355_bfv_unpack_bytes_ntt for N >= 2048: the forward COLUMN pass of plaintext j's transform, structured as
//                        k_bfv_digits_cols_fwd.  A block owns a quarter of the 1024 columns of one plaintext; a lane owns one stride-1024
//                        column: it cuts its N / 1024 fields out of the byte string once and keeps them in registers; then, per output
//                        prime i' < L_out, it lifts them centred (bfv_lift_centred), runs k_cols_fwd's lane program with the engine that
//                        owns i' (fp64 or u64, the u64 one in this build's form) and stores the raw column into out(j, i').  The row pass
//                        is the existing k_rows_fwd, in place.  Neither the [n][N] coefficient slab nor the lifted slab exists.  The four
//                        blocks of a plaintext are neighbours in the grid and read the same words.  N = 1024 has no column pass: the
//                        caller runs the two-call composition.
// Launches: kernel_common.inc's dispatch_logn1 picks the LOGN1 instantiation, streaming_grid / grid_blocks size and bound the grids.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "bfv_bytes_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_bytes.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// bytes: plaintext j at bytes + j stride, B bytes; words: [n][N] coefficients or [n][L_out][N] transformed
struct BfvBytesArgs {
    const unsigned char *bytes_in; // unpack: the source
    unsigned char *bytes_out;      // pack: the target (8-byte aligned, stride a multiple of 8)
    const u64 *in;                 // pack: the coefficients
    u64 *out;                      // unpack: the coefficients / the transformed plaintexts
    u64 n, stride, B, t;
    int w, logN, L_out;
};

__global__ void __launch_bounds__(kBlock) k_bfv_unpack(BfvBytesArgs A)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 j = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (j >= A.n) return;
    const BfvByteSrc s = bfv_bytes_src(A.bytes_in + j * A.stride, A.B);
    reinterpret_cast<ulonglong2 *>(A.out + (j << A.logN))[e2] = make_ulonglong2(bfv_bytes_field(s, 2 * e2, A.w), bfv_bytes_field(s, 2 * e2 + 1, A.w));
}

__global__ void __launch_bounds__(kBlock) k_bfv_pack(BfvBytesArgs A)
{
    const u64 j = blockIdx.x, k = (u64)blockIdx.y * kBlock + threadIdx.x; // (a plaintext per grid column: no division by the word count)
    if (k >= bfv_bytes_words(A.B)) return;
    reinterpret_cast<u64 *>(A.bytes_out + j * A.stride)[k] = bfv_bytes_pack_word(A.in + (j << A.logN), (u64)1 << A.logN, k, A.B, A.w);
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_bytes_cols_fwd(BfvBytesArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 j = blockIdx.x >> 2; // the plaintext
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const BfvByteSrc s = bfv_bytes_src(A.bytes_in + j * A.stride, A.B);
    u64 fld[N1];
#pragma unroll
    for (int a = 0; a < N1; ++a) fld[a] = bfv_bytes_field(s, (u64)((a << kRowLog) + col), A.w);
    for (int ip = 0; ip < A.L_out; ++ip) {
        const PrimeDev &P = primes[ip];
        const ModU64 mi = make_modu(P);
        u64 *dst = A.out + ((j * A.L_out + ip) << (LOGN1 + kRowLog));
        if (P.f64) {
            const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
            double x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(bfv_lift_centred(fld[a], A.t, mi));
            col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
        } else {
            const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
            u64 x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = bfv_lift_centred(fld[a], A.t, mi);
            col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
        }
    }
}

BfvBytesArgs bytes_args(const KernelEnv &env, int w, u64 n, u64 stride, u64 B)
{
    const u64 N = (u64)1 << (env.logn1 + kRowLog);
    if (w < 1 || w > 63 || B < 1 || B > bfv_bytes_max(N, w) || stride < B) throw std::invalid_argument("database bytes: field width, byte count or stride out of range");
    BfvBytesArgs A{};
    A.n = n; A.stride = stride; A.B = B; A.w = w; A.logN = env.logn1 + kRowLog;
    return A;
}
unsigned grid_of(u64 blocks) { return grid_blocks(blocks, "database bytes", "plaintexts"); }

} // namespace

void launch_bfv_unpack(const KernelEnv &env, int w, u64 n, const void *bytes, u64 stride, u64 B, u64 *plain)
{
    if (!n) return;
    BfvBytesArgs A = bytes_args(env, w, n, stride, B);
    A.bytes_in = static_cast<const unsigned char *>(bytes); A.out = plain;
    hipLaunchKernelGGL(k_bfv_unpack, dim3(streaming_grid(n, A.logN, "database bytes", "plaintexts")), dim3(kBlock), 0, env.stream, A);
}
void launch_bfv_pack(const KernelEnv &env, int w, u64 n, const u64 *plain, u64 B, u64 stride, void *bytes)
{
    if (!n) return;
    BfvBytesArgs A = bytes_args(env, w, n, stride, B);
    if (((unsigned long long)bytes & 7) || (stride & 7) || stride < 8 * bfv_bytes_words(B))
        throw std::invalid_argument("database bytes: the packed side must be 8-byte aligned, its stride a multiple of 8 that holds the last word");
    A.in = plain; A.bytes_out = static_cast<unsigned char *>(bytes);
    hipLaunchKernelGGL(k_bfv_pack, dim3(grid_of(n), (unsigned)((bfv_bytes_words(B) + kBlock - 1) / kBlock)), dim3(kBlock), 0, env.stream, A);
}
void launch_bfv_bytes_cols_fwd(const KernelEnv &env, int w, u64 n, const void *bytes, u64 stride, u64 B, int L_out, u64 t, u64 *out)
{
    if (!n) return;
    if (env.logn1 == 0) throw std::invalid_argument("database bytes: N = 1024 has no column pass");
    if (L_out < 1 || L_out > kMaxPrimes) throw std::invalid_argument("database bytes: output level out of range");
    BfvBytesArgs A = bytes_args(env, w, n, stride, B);
    A.bytes_in = static_cast<const unsigned char *>(bytes); A.out = out; A.L_out = L_out; A.t = t;
    const dim3 g(grid_of(n * 4)), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_bfv_bytes_cols_fwd<decltype(n1)::value>, g, b, 0, env.stream, A, env.primes); });
}

} // namespace HE355_KNS
} // namespace he355
