// he355_kernels_bfv_gadget.hip -- the BFV external product RGSW(m) [.] BFV(mu) -> BFV(m mu): he355_bfv_gadget_decompose_ntt,
// he355_bfv_rgsw_encrypt, he355_bfv_external_product.  The per-coefficient arithmetic is bfv_gadget_core.h and bfv_mac_core.h
// (host-compilable: tests/csim/sim_bfv_gadget.cpp runs the same text on the CPU).
//
//   k_bfv_gadget_cols_fwd<LOGN1>   N >= 2048: the forward COLUMN pass of every digit polynomial of one ciphertext residue.  A block owns a
//                        quarter of the 1024 columns of one residue polynomial (c, k, i); a lane owns one stride-1024 column and loads its
//                        N / 1024 ciphertext words ONCE.  For each digit g < E_i and each output prime j < L it cuts the digit (the plain
//                        integer below 2^v, reduced once where it is not below q_j), runs k_cols_fwd's lane program with the engine that
//                        owns j (fp64 or u64, the u64 one in this build's form) and stores the raw column into digit polynomial
//                        (c 2E + k E + off_i + g, j).  The row pass is the existing k_rows_fwd, in place.  Registers: the N / 1024 source
//                        words and one working column, as k_bfv_digits_cols_fwd.  The ciphertexts are read where they lie: ciphertext
//                        (a, b) at index a stride_a + b stride_b.
//   k_bfv_gadget_spread  N = 1024 (no column pass) and batches too small to fill the chip with column-pass blocks: streaming; a lane owns two
//                        coefficients of one residue polynomial, one 16-byte load, E_i L 16-byte stores of the digits under every output prime, coefficient form; the existing transform follows in place.
//   k_bfv_gadget_mac     batched over results; a lane owns two coefficients (16 bytes per access) of residue j of result r, both
//                        polynomials.  Per term (kappa, f) it loads one digit word and two RGSW row words and feeds four 128-bit sums,
//                        folded per bfv_mac_run of prime j; canonical residues out.  Block = (residue, coefficient block, result), the
//                        result fastest: with one selector row for all results (rg_stride_r == 0) the blocks that read the same row
//                        words are neighbours in the grid, as in k_bfv_plain_mac.
//   k_bfv_rgsw_plant     streaming; a lane owns two coefficients of one output residue polynomial (row, k', i'): it reads the encryption of
//                        zero (level L_in >= L, cut to the first L primes) and, where (k', i') is the row's own (k, i), adds
//                        lift(m) 2^(g v) mod q_i.  In place when L_in == L.  The existing forward transform follows.
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>

#include "he355_kernels.h"
#include "bfv_gadget_core.h"
#include "bfv_mac_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_gadget.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// ciphertext (a, b), a < n_a, b < n_b, at index a stride_a + b stride_b of `in`, [size][L][N] each; digit polynomials
// [(a n_b + b) size E + f][L][N] of `out`
struct BfvGadgetCutArgs {
    const u64 *in;
    u64 *out;
    u64 n_b, stride_a, stride_b;
    u64 n_polys; // n_a n_b size L residue polynomials
    int L, size, logN;
    BfvDigitTab tab;
};

// residue polynomial p of the batch -> its words
__device__ __forceinline__ const u64 *gadget_src(const BfvGadgetCutArgs &A, u64 p)
{
    const u64 polys = (u64)A.size * A.L, c = p / polys, rest = p % polys;
    const u64 at = (c / A.n_b) * A.stride_a + (c % A.n_b) * A.stride_b;
    return A.in + ((at * polys + rest) << A.logN);
}

template <int LOGN1>
__global__ void __launch_bounds__(kBlock) k_bfv_gadget_cols_fwd(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    constexpr int N1 = 1 << LOGN1;
    const u64 p = blockIdx.x >> 2; // residue polynomial (c size + k) L + i
    const int col = ((blockIdx.x & 3) << 8) | threadIdx.x;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, A.size, p);
    const u64 *src = gadget_src(A, p);
    u64 w[N1];
#pragma unroll
    for (int a = 0; a < N1; ++a) w[a] = src[(a << kRowLog) + col];
    for (int g = 0; g < E; ++g) {
        for (int j = 0; j < A.L; ++j) {
            const PrimeDev &P = primes[j];
            const ModU64 mj = make_modu(P);
            u64 *dst = A.out + (((f0 + g) * A.L + j) << (LOGN1 + kRowLog));
            if (P.f64) {
                const ArF64 ar = make_ar(P, (ArF64 *)nullptr);
                double x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = ar.from_canon(bfv_gadget_digit(w[a], g, v, mj));
                col_fwd<ArF64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = ar.to_raw(x[a]);
            } else {
                const ArU64 ar = make_ar(P, (ArU64 *)nullptr);
                u64 x[N1];
#pragma unroll
                for (int a = 0; a < N1; ++a) x[a] = bfv_gadget_digit(w[a], g, v, mj);
                col_fwd<ArU64, LOGN1>(ar, x, ctw(P.fwd));
#pragma unroll
                for (int a = 0; a < N1; ++a) dst[(a << kRowLog) + col] = x[a];
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) k_bfv_gadget_spread(BfvGadgetCutArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const int i = (int)(p % (u64)A.L), E = A.tab.D[i], v = A.tab.w;
    const u64 f0 = bfv_gadget_first(A.tab, A.size, p);
    const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(gadget_src(A, p))[e2];
    for (int g = 0; g < E; ++g)
        for (int j = 0; j < A.L; ++j) {
            const ModU64 mj = make_modu(primes[j]);
            reinterpret_cast<ulonglong2 *>(A.out + (((f0 + g) * A.L + j) << A.logN))[e2] =
                make_ulonglong2(bfv_gadget_digit(x.x, g, v, mj), bfv_gadget_digit(x.y, g, v, mj));
        }
}

// result r < n: digits [r][inner][rows][L][N] (NTT form), RGSW (r, kappa) at index r rg_stride_r + kappa rg_stride_k, [rows][2][L][N] each
struct BfvGadgetMacArgs {
    const u64 *dig, *rgsw;
    u64 *out;
    u64 n, rg_stride_r, rg_stride_k;
    u32 inner, rows, pairs_blocks; // rows = 2 E(L); pairs_blocks = N / 2 / kBlock
    int L, logN;
    u32 run[kMaxPrimes]; // bfv_mac_run of prime j
};

__global__ void __launch_bounds__(kBlock) k_bfv_gadget_mac(BfvGadgetMacArgs A, const PrimeDev *primes)
{
    // block = (residue j, coefficient block, result), the result fastest
    const u64 r = blockIdx.x % A.n;
    const u32 rest = (u32)(blockIdx.x / A.n), eb = rest % A.pairs_blocks;
    const int j = (int)(rest / A.pairs_blocks);
    const u64 e2 = (u64)eb * kBlock + threadIdx.x;
    const u64 N = (u64)1 << A.logN, LN = (u64)A.L << A.logN;
    const ModU64 m = bfv_modu(primes[j]);
    const u64 run = A.run[j];
    // in 16-byte words: a digit polynomial is LN / 2 after the one before it, an RGSW row LN, its second polynomial LN / 2 into the row
    const ulonglong2 *pd = reinterpret_cast<const ulonglong2 *>(A.dig + r * A.inner * A.rows * LN + (u64)j * N) + e2;
    const ulonglong2 *pr = reinterpret_cast<const ulonglong2 *>(A.rgsw + r * A.rg_stride_r * A.rows * 2 * LN + (u64)j * N) + e2;
    const u64 step_k = A.rg_stride_k * A.rows * LN, half = LN / 2;

    u128 acc[2][2] = {{0, 0}, {0, 0}}; // [polynomial][coefficient]
    u64 left = run;                    // terms the running sums still take
    for (u32 kappa = 0; kappa < A.inner; ++kappa) {
        const ulonglong2 *row = pr + kappa * step_k;
        u32 f = 0;
        while (f < A.rows) {
            if (!left) { // the sums' residues start the next run as one term
                bfv_mac_fold(acc[0][0], m); bfv_mac_fold(acc[0][1], m);
                bfv_mac_fold(acc[1][0], m); bfv_mac_fold(acc[1][1], m);
                left = run - 1;
            }
            const u32 end = A.rows - f < left ? A.rows : f + (u32)left;
            left -= end - f;
#pragma unroll 2
            for (; f < end; ++f) {
                const ulonglong2 d = pd[f * half], a = row[f * LN], b = row[f * LN + half];
                bfv_mac_add(acc[0][0], a.x, d.x);
                bfv_mac_add(acc[0][1], a.y, d.y);
                bfv_mac_add(acc[1][0], b.x, d.x);
                bfv_mac_add(acc[1][1], b.y, d.y);
            }
        }
        pd += A.rows * half;
    }
    ulonglong2 *po = reinterpret_cast<ulonglong2 *>(A.out + r * 2 * LN + (u64)j * N) + e2;
    po[0] = make_ulonglong2(bfv_mac_reduce(acc[0][0], m), bfv_mac_reduce(acc[0][1], m));
    po[half] = make_ulonglong2(bfv_mac_reduce(acc[1][0], m), bfv_mac_reduce(acc[1][1], m));
}

// zero [n_rows][2][L_in][N] (encryptions of zero, coefficient form), plain [n][N] mod t -> out [n_rows][2][L][N], n_rows = n 2 E(L)
struct BfvPlantArgs {
    const u64 *zero, *plain;
    u64 *out;
    u64 n_polys; // n_rows 2 L output residue polynomials
    u64 t;
    int L, L_in, logN;
    BfvDigitTab tab;
};

__global__ void __launch_bounds__(kBlock) k_bfv_rgsw_plant(BfvPlantArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 row = p / (2 * (u64)A.L);
    const int kk = (int)((p / (u64)A.L) & 1), ii = (int)(p % (u64)A.L);
    const BfvDigitSrc s = bfv_gadget_src(A.tab, 2, row); // row = r 2E + k E + off_i + g; s.poly = (2 r + k) L + i
    ulonglong2 x = reinterpret_cast<const ulonglong2 *>(A.zero + (((row * 2 + kk) * A.L_in + ii) << A.logN))[e2];
    if (s.prime == ii && (int)((s.poly / (u64)A.L) & 1) == kk) {
        const ModU64 mi = make_modu(primes[ii]);
        const ulonglong2 mm = reinterpret_cast<const ulonglong2 *>(A.plain + ((s.poly / (2 * (u64)A.L)) << A.logN))[e2];
        x.x = addmod(x.x, bfv_gadget_plant(mm.x, A.t, s.digit, A.tab.w, mi), mi.q);
        x.y = addmod(x.y, bfv_gadget_plant(mm.y, A.t, s.digit, A.tab.w, mi), mi.q);
    }
    reinterpret_cast<ulonglong2 *>(A.out + (p << A.logN))[e2] = x;
}

BfvGadgetCutArgs cut_args(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *in, u64 stride_a, u64 stride_b, u64 *out)
{
    if (L < 1 || L > kMaxPrimes || tab.L != L || size < 1 || size > 3 || !bfv_gadget_width_ok(tab.w))
        throw std::invalid_argument("gadget decomposition: level, size or digit table out of range");
    BfvGadgetCutArgs A{};
    A.in = in; A.out = out; A.n_b = n_b; A.stride_a = stride_a; A.stride_b = stride_b;
    A.n_polys = n_a * n_b * size * L; A.L = L; A.size = size; A.logN = env.logn1 + kRowLog; A.tab = tab;
    return A;
}
unsigned streaming_grid(u64 n_polys, int logN, const char *what)
{
    const u64 blocks = (n_polys << (logN - 1)) / kBlock; // N / 2 is a multiple of kBlock: a block lies inside one polynomial
    if (blocks > 0x7fffffffull) throw std::invalid_argument(std::string(what) + ": too many polynomials for one launch");
    return (unsigned)blocks;
}

} // namespace

void launch_bfv_gadget_cut(const KernelEnv &env, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out, bool cols)
{
    if (!n_a || !n_b) return;
    const BfvGadgetCutArgs A = cut_args(env, tab, L, size, n_a, n_b, ct, stride_a, stride_b, out);
    if (env.logn1 == 0 && cols) throw std::invalid_argument("gadget decomposition: N = 1024 has no column pass");
    if (!cols) {
        hipLaunchKernelGGL(k_bfv_gadget_spread, dim3(streaming_grid(A.n_polys, A.logN, "gadget decomposition")), dim3(kBlock), 0, env.stream, A, env.primes);
        return;
    }
    const u64 blocks = A.n_polys * 4;
    if (blocks > 0x7fffffffull) throw std::invalid_argument("gadget decomposition: too many polynomials for one launch");
    const dim3 g((unsigned)blocks), b(kBlock);
    switch (env.logn1) {
    case 1: hipLaunchKernelGGL(k_bfv_gadget_cols_fwd<1>, g, b, 0, env.stream, A, env.primes); break;
    case 2: hipLaunchKernelGGL(k_bfv_gadget_cols_fwd<2>, g, b, 0, env.stream, A, env.primes); break;
    case 3: hipLaunchKernelGGL(k_bfv_gadget_cols_fwd<3>, g, b, 0, env.stream, A, env.primes); break;
    case 4: hipLaunchKernelGGL(k_bfv_gadget_cols_fwd<4>, g, b, 0, env.stream, A, env.primes); break;
    case 5: hipLaunchKernelGGL(k_bfv_gadget_cols_fwd<5>, g, b, 0, env.stream, A, env.primes); break;
    default: throw std::invalid_argument("ring size out of range");
    }
}
static u64 gadget_mac_blocks(const KernelEnv &env, int L, u64 n) { return n * (u64)L * ((((u64)1 << (env.logn1 + kRowLog)) / 2) / kBlock); }
void launch_bfv_gadget_mac(const KernelEnv &env, int L, u64 n, u64 inner, u32 rows, const u64 *dig, const u64 *rgsw, u64 rg_stride_r, u64 rg_stride_k, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || inner < 1 || rows < 2 || inner * rows > 0x7fffffffull)
        throw std::invalid_argument("he355_bfv_external_product: level or inner dimension out of range");
    BfvGadgetMacArgs A{};
    A.dig = dig; A.rgsw = rgsw; A.out = out; A.n = n; A.rg_stride_r = rg_stride_r; A.rg_stride_k = rg_stride_k;
    A.inner = (u32)inner; A.rows = rows; A.L = L; A.logN = env.logn1 + kRowLog;
    A.pairs_blocks = (u32)((((u64)1 << A.logN) / 2) / kBlock);
    for (int j = 0; j < L; ++j) {
        A.run[j] = (u32)bfv_mac_run(env.prime_q[j]);
        if (A.run[j] < 2) throw std::invalid_argument("he355_bfv_external_product: prime too wide for a 128-bit sum");
    }
    const u64 blocks = gadget_mac_blocks(env, L, n);
    if (blocks > 0x7fffffffull) throw std::invalid_argument("he355_bfv_external_product: too many results for one launch");
    hipLaunchKernelGGL(k_bfv_gadget_mac, dim3((unsigned)blocks), dim3(kBlock), 0, env.stream, A, env.primes);
}
void launch_bfv_rgsw_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, int L_in, u64 n, const u64 *zero, const u64 *plain, u64 t, u64 *out)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || tab.L != L || L_in < L || !bfv_gadget_width_ok(tab.w)) throw std::invalid_argument("he355_bfv_rgsw_encrypt: level or digit table out of range");
    BfvPlantArgs A{};
    A.zero = zero; A.plain = plain; A.out = out; A.n_polys = n * 2 * tab.total * 2 * L; A.t = t; A.L = L; A.L_in = L_in; A.logN = env.logn1 + kRowLog; A.tab = tab;
    hipLaunchKernelGGL(k_bfv_rgsw_plant, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_rgsw_encrypt")), dim3(kBlock), 0, env.stream, A, env.primes);
}

} // namespace HE355_KNS
} // namespace he355
