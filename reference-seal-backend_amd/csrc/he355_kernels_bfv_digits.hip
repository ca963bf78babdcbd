// he355_kernels_bfv_digits.hip -- the cut of coefficient-form BFV ciphertexts into plaintexts and its inverse, the step between the two
// scans of a recursive (two-dimensional) PIR: he355_bfv_decompose, he355_bfv_decompose_ntt, he355_bfv_compose.  The per-coefficient arithmetic
// is bfv_digits_core.h (host-compilable: tests/csim/sim_bfv_digits.cpp runs the same text on the CPU) and bfv_level_core.h's centred lift.
//
//   k_bfv_digits         streaming; a lane owns two neighbouring coefficients of one residue polynomial (k, i) of one ciphertext: one 16-byte
//                        load, D_i 16-byte stores, digit g into plaintext r F + k D(L) + off_i + g.  Each ciphertext word is read once.
//   k_bfv_undigits       the inverse; a lane owns two coefficients of one residue polynomial of the result: D_i 16-byte loads, the masked
//                        digits summed at their places, one conditional subtraction, one 16-byte store.
//   k_bfv_digits_cols_fwd<LOGN1>   he355_bfv_decompose_ntt for N >= 2048: the forward COLUMN pass of plaintext f's transform, reading the
//                        ciphertext residue out of place as k_bfv_mp_cols_fwd reads `ct`.  A block owns a quarter of the 1024 columns of one
//                        plaintext f = (r, k, i, g); a lane owns one stride-1024 column: it loads its N / 1024 ciphertext words once, cuts
//                        digit g out of each and keeps the digits in registers; then, per output prime i' < L_out, it lifts them centred
//                        (bfv_lift_centred: exactly the canonical residues k_bfv_lift_plain would have stored), runs k_cols_fwd's lane
//                        program with the engine that owns i' (fp64 or u64, the u64 one in this build's form) and stores the raw column into
//                        out(f, i').  The row pass is the existing k_rows_fwd, in place.  Neither the [n][F][N] plaintext slab nor the lifted
//                        [n][F][L_out][N] slab is written or read back.  The D_i blocks that share a ciphertext residue are neighbours in
//                        the grid, so the word leaves HBM once.  N = 1024 has no column pass: the caller runs the two-call composition.
// Launches: kernel_common.inc's dispatch_logn1 picks the LOGN1 instantiation, streaming_grid / grid_blocks size and bound the grids.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "bfv_digits_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_digits.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// ciphertexts [n][size][L][N]; plaintexts [n][F][N] (coefficients) or [n][F][L_out][N] (transformed), F = size D(L)
struct BfvDigitsArgs {
    const u64 *in;
    u64 *out;
    u64 n_polys; // streaming kernels: n size L residue polynomials of the ciphertext side
    u64 t;       // fused column pass: the plain modulus
    int L, size, logN, L_out;
    BfvDigitTab tab;
};

__global__ void __launch_bounds__(kBlock) k_bfv_digits(BfvDigitsArgs A)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 poly = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (poly >= A.n_polys) return;
    const int polys = A.size * A.L, p = (int)(poly % polys), k = p / A.L, i = p % A.L;
    const u64 r = poly / polys;
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.in + (poly << A.logN))[e2];
    const u64 f0 = (r * A.size + k) * A.tab.total + A.tab.off[i];
    const int D = A.tab.D[i], w = A.tab.w;
    for (int g = 0; g < D; ++g)
        reinterpret_cast<ulonglong2 *>(A.out + ((f0 + g) << A.logN))[e2] = make_ulonglong2(bfv_digit(x.x, g, w), bfv_digit(x.y, g, w));
}

__global__ void __launch_bounds__(kBlock) k_bfv_undigits(BfvDigitsArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 poly = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (poly >= A.n_polys) return;
    const int polys = A.size * A.L, p = (int)(poly % polys), k = p / A.L, i = p % A.L;
    const u64 r = poly / polys;
    const u64 f0 = (r * A.size + k) * A.tab.total + A.tab.off[i];
    const int D = A.tab.D[i], w = A.tab.w, b = A.tab.bits[i];
    const u64 q = primes[i].q;
    u64 sx = 0, sy = 0;
    for (int g = 0; g < D; ++g) {
        const ulonglong2 d = reinterpret_cast<const ulonglong2 *>(A.in + ((f0 + g) << A.logN))[e2];
        sx += bfv_undigit_term(d.x, g, D, b, w);
        sy += bfv_undigit_term(d.y, g, D, b, w);
    }
    reinterpret_cast<ulonglong2 *>(A.out + (poly << A.logN))[e2] = make_ulonglong2(bfv_undigit_finish(sx, q), bfv_undigit_finish(sy, q));
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_digits_cols_fwd(BfvDigitsArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 pf = blockIdx.x >> 2; // plaintext r F + f
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const BfvDigitSrc s = bfv_digit_src(A.tab, A.size, pf);
    const int g = s.digit, w = A.tab.w;
    const u64 *src = A.in + (s.poly << (LOGN1 + kRowLog));
    u64 dig[N1];
#pragma unroll
    for (int a = 0; a < N1; ++a) dig[a] = bfv_digit(src[(a << kRowLog) + col], g, w);
    for (int ip = 0; ip < A.L_out; ++ip) {
        const PrimeDev &P = primes[ip];
        const ModU64 mi = make_modu(P);
        u64 *dst = A.out + ((pf * A.L_out + ip) << (LOGN1 + kRowLog));
        if (P.f64) {
            const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
            double x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(bfv_lift_centred(dig[a], A.t, mi));
            col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
        } else {
            const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
            u64 x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = bfv_lift_centred(dig[a], A.t, mi);
            col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
            for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
        }
    }
}

BfvDigitsArgs digits_args(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *in, u64 *out)
{
    if (L < 1 || L > kMaxPrimes || tab.L != L || size < 1 || size > 3 || tab.w < 1 || tab.w > 63)
        throw std::invalid_argument("ciphertext decomposition: level, size or digit table out of range");
    BfvDigitsArgs A{};
    A.in = in; A.out = out; A.n_polys = n * size * L; A.L = L; A.size = size; A.logN = env.logn1 + kRowLog; A.tab = tab;
    return A;
}

} // namespace

void launch_bfv_digits(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *ct, u64 *plain)
{
    if (!n) return;
    const BfvDigitsArgs A = digits_args(env, tab, L, size, n, ct, plain);
    hipLaunchKernelGGL(k_bfv_digits, dim3(streaming_grid(A.n_polys, A.logN, "ciphertext decomposition")), dim3(kBlock), 0, env.stream, A);
}
void launch_bfv_undigits(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *plain, u64 *ct)
{
    if (!n) return;
    const BfvDigitsArgs A = digits_args(env, tab, L, size, n, plain, ct);
    hipLaunchKernelGGL(k_bfv_undigits, dim3(streaming_grid(A.n_polys, A.logN, "ciphertext decomposition")), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bfv_digits_cols_fwd(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n, const u64 *ct, int L_out, u64 t, u64 *out)
{
    if (!n) return;
    if (env.logn1 == 0) throw std::invalid_argument("ciphertext decomposition: N = 1024 has no column pass");
    if (L_out < 1 || L_out > kMaxPrimes) throw std::invalid_argument("ciphertext decomposition: output level out of range");
    BfvDigitsArgs A = digits_args(env, tab, L, size, n, ct, out);
    A.L_out = L_out; A.t = t;
    const dim3 g(grid_blocks(n * size * tab.total * 4, "ciphertext decomposition", "plaintexts")), b(kBlock);
    dispatch_logn1(env.logn1, [&](auto n1) { hipLaunchKernelGGL(k_bfv_digits_cols_fwd<decltype(n1)::value>, g, b, 0, env.stream, A, env.primes); });
}

} // namespace HE355_KNS
} // namespace he355
