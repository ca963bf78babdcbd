// he355_kernels_raise.hip -- the CKKS modulus raise (he355_ckks_mod_raise, he355_ckks_lift_centred): the residue under q_0 of a polynomial,
// read as centred integers, re-expressed under q_0 .. q_{L_to - 1}.  The per-coefficient arithmetic is raise_core.h (host-compilable:
// tests/csim/sim_raise.cpp runs the same text on the CPU).
//
//   k_raise_lift         streaming, 16-byte accesses; a lane owns two neighbouring coefficients of one source polynomial ([n_polys][N],
//                        canonical under q_0): one load, one store per target row `first` .. L_to - 1 of out [n_polys][L_to][N], the canonical
//                        c mod q_j in coefficient form (integers for every prime: all residues are u64 words in HBM in both engines).
//                        he355_ckks_lift_centred (first = 0), and the raise at N = 1024, which has no column pass (first = 1).
//   k_raise_cols<LOGN1>  the fused route for N >= 2048, after k_rows_inv_select wrote the tail [n_polys][N] (raw rows of prime 0).  A block
//                        owns a quarter of the 1024 columns of one polynomial, a lane one stride-1024 column: it finishes the inverse
//                        transform under q_0 (col_inv, in the engine that owns prime 0, as floor_source_column does), canonicalises and keeps
//                        the N / 1024 sources in registers (N = 32768: parked in LDS, see PARK); then, per target j >= 1, it reduces them into q_j in the target's engine, runs
//                        k_cols_fwd's lane program and stores the raw column into row j of out.  The row pass is the existing k_rows_fwd,
//                        in place.  Neither the coefficient slab nor the lifted [L_to][N] slab exists.  tsplit > 1 (small batches): the
//                        targets of a column are dealt to tsplit blocks along blockIdx.y, each of which redoes the source column.
// Launches: kernel_common.inc's dispatch_logn1 picks the LOGN1 instantiation, streaming_grid / grid_blocks size and bound the grids.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "raise_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_raise.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

struct RaiseArgs {
    const u64 *src; // k_raise_lift: coefficients [n_polys][N]; k_raise_cols: the tail [n_polys][N], raw rows of prime 0
    u64 *out;       // [n_polys][L_to][N]
    u64 n_polys;
    int L_to, first, logN, tsplit;
};

__global__ void __launch_bounds__(kBlock) k_raise_lift(RaiseArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1);
    if (p >= A.n_polys) return; // (a block lies inside one polynomial: the whole block leaves)
    const u64 e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    const u64 q0 = primes[0].q;
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.src + (p << A.logN))[e2];
    for (int j = A.first; j < A.L_to; ++j) {
        const ModU64 mj = make_modu(primes[j]);
        reinterpret_cast<ulonglong2 *>(A.out + ((p * (u64)A.L_to + (u64)j) << A.logN))[e2] = make_ulonglong2(raise_lift_u64(x.x, q0, mj), raise_lift_u64(x.y, q0, mj));
    }
}

// source a of the lane's column: parked in LDS or register c[a].  The parked word is read through an LDS-qualified volatile pointer: a
// ds_read whatever the compiler can prove about the address, and one per use -- the read stays inside the loop over the targets instead of
// being hoisted back into registers, which is the whole point of parking.  That is a property of the generated code, not of the language:
// after a toolchain change re-check tools/kres.py for k_raise_cols<5> (122 VGPRs, 65536 bytes of LDS, no spill, no scratch) before the
// figures of profiles/ckks_mod_raise.txt are relied on.
typedef const volatile __attribute__((address_space(3))) u64 *lds_cvu64_t;
template <bool PARK> __device__ __forceinline__ u64 raise_source(const u64 *mine, const u64 *c, int a)
{
    if constexpr (PARK) return ((lds_cvu64_t)mine)[a * kBlock];
    else return c[a];
}

// PARK (LOGN1 = 5): the 32 sources wait in LDS, [N1][kBlock] words (64 KiB), each lane reading back only what it wrote itself (no barrier) --
// source and working column together take 352 registers and one wave per SIMD; parked, 122 and two.  Measured at N = 2^15, 1 -> 16, n = 64:
// 241 -> 173 us (profiles/ckks_mod_raise.txt).  At LOGN1 = 4 both fit two waves per SIMD as they are, and parking them measured 3-5 % slower.
template <int LOGN1>
__global__ void __launch_bounds__(kBlock, LOGN1 >= 5 ? 2 : 1) k_raise_cols(RaiseArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    constexpr bool PARK = LOGN1 >= 5;
    __shared__ u64 park[PARK ? N1 : 1][PARK ? kBlock : 1];
    const u64 poly = blockIdx.x >> 2;
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const PrimeDev &P0 = primes[0];
    const u64 q0 = P0.q;
    const u64 *src = A.src + (poly << (LOGN1 + kRowLog));
    u64 c[N1]; // the column's coefficients, canonical under q_0
    if (P0.f64) {
        const ArF64 ar = make_ar(P0, (ArF64 *)nullptr);
        double x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, x, ctw(P0.inv), P0.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    } else {
        const ArU64 ar = make_ar(P0, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(P0.inv), P0.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
    }
    if constexpr (PARK) {
#pragma unroll
        for (int a = 0; a < N1; ++a) park[a][threadIdx.x] = c[a];
    }
    const u64 *mine = &park[0][PARK ? threadIdx.x : 0];
    const bool wide = (q0 >> 52) != 0;
    for (int j = raise_first_target((int)blockIdx.y); j < A.L_to; j += A.tsplit) {
        const PrimeDev &P = primes[j];
        u64 *dst = A.out + ((poly * (u64)A.L_to + (u64)j) << (LOGN1 + kRowLog));
        if (P.f64) {
            const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
            double x[N1];
            if (wide) {
                const double pow32 = P.pow32;
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = raise_lift_f64_wide(ar, raise_source<PARK>(mine, c, a), q0, pow32);
            } else {
                const bool rc = raise_recentre(q0, P.q);
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = raise_lift_f64(ar, raise_centre_f64(raise_source<PARK>(mine, c, a), q0), rc);
            }
            col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
        } else {
            const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
            const ModU64 mj = make_modu(P);
            u64 x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = raise_lift_u64(raise_source<PARK>(mine, c, a), q0, mj);
            col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
        }
    }
}

RaiseArgs raise_args(const KernelEnv &env, int L_to, int first, u64 n_polys, const u64 *src, u64 *out)
{
    if (L_to < 1 || L_to > kMaxPrimes || L_to > env.K || first < 0 || first > 1 || !src || !out)
        throw std::invalid_argument("modulus raise: the launch needs a target level of the chain and its buffers");
    RaiseArgs A{};
    A.src = src; A.out = out; A.n_polys = n_polys; A.L_to = L_to; A.first = first; A.logN = env.logn1 + kRowLog; A.tsplit = 1;
    return A;
}

} // namespace

void launch_raise_lift(const KernelEnv &env, int L_to, int first, u64 n_polys, const u64 *coeff, u64 *out)
{
    if (!n_polys || first >= L_to) return;
    const RaiseArgs A = raise_args(env, L_to, first, n_polys, coeff, out);
    hipLaunchKernelGGL(k_raise_lift, dim3(streaming_grid(n_polys, A.logN, "modulus raise")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_raise_cols(const KernelEnv &env, int L_to, u64 n_polys, const u64 *tail, u64 *out, int tsplit)
{
    if (!n_polys || L_to < 2) return;
    if (env.logn1 == 0) throw std::invalid_argument("modulus raise: N = 1024 has no column pass");
    RaiseArgs A = raise_args(env, L_to, 1, n_polys, tail, out);
    if (tsplit < 1 || tsplit > L_to - 1) throw std::invalid_argument("modulus raise: a column's targets are dealt to 1 .. L_to - 1 blocks (raise_tsplit)");
    A.tsplit = tsplit;
    const dim3 g(grid_blocks(n_polys * 4, "modulus raise"), (unsigned)A.tsplit), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_raise_cols<decltype(n1)::value>, g, b, 0, env.stream, A, env.primes); });
}

} // namespace HE355_KNS
} // namespace he355
