// he355_kernels_bfv_seeded.hip -- seeded (secret-key) BFV queries and seeded Galois keys: he355_bfv_seeded_encrypt,
// he355_bfv_seeded_selector_encrypt, he355_bfv_seeded_restore, he355_keygen_galois_seeded, he355_set_galois_key_seeded.  The per-coefficient
// arithmetic is bfv_seeded_core.h (host-compilable: tests/csim/sim_bfv_seeded.cpp runs the same text on the CPU); the transforms are the
// existing launch_ntt_*.
//
//   k_bfv_seeded_gen<MUL>  the uniform half a ciphertext or a key digit carries as a seed, NTT form.  Streaming: a lane owns two
//                        neighbouring coefficients of one residue polynomial (item, i) and stores them as 16 bytes; the polynomial's stream,
//                        its base word, the prime's Barrett words and its acceptance limit are block-uniform (a block lies inside one
//                        polynomial).  Per coefficient: one splitmix64 and one barrett64 on the straight path, draws 2..8 in a rarely
//                        taken branch.  This is the server's per-query kernel (he355_bfv_seeded_restore, he355_set_galois_key_seeded).
//                        MUL (the client): the product with the NTT-form secret key is stored instead, a never reaches memory.
//   k_bfv_seeded_finish  the client: c0 = Delta_L(m) - e - w per prime, w = iNTT(a (.) s) read from scratch; a lane owns two coefficients
//                        of one ciphertext and all its L residues, so e (one draw per coefficient) and Delta's shared part are formed once
//                        and neither is stored.
//   k_bfv_seeded_place   c0 [n][L][N] -> polynomial 0 of out [n][2][L][N], 16 bytes per lane.
//   k_bfv_seeded_plant   the selectors of he355_bfv_selector_encrypt added in place to c0 [n][L][N]: k_bfv_selector_plant's plant on a slab
//                        that has no polynomial 1 (that kernel's strides are [n][2][L_in][N] and [n][2][L][N]).
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <type_traits>

#include "he355_kernels.h"
#include "bfv_seeded_core.h"
#include "ntt_core.h"

#if !defined(HE355_KNS) || !defined(HE355_U64_FOLD)
#error "he355_kernels_bfv_seeded.hip is compiled once per form of the u64 engine (Makefile)"
#endif
namespace he355 {
namespace HE355_KNS {
namespace {

#include "kernel_common.inc"

// polynomial (item, i), i < polys: stream stream0 + item stream_step + i, prime i, words out + item item_stride + i N
struct BfvSeededGenArgs {
    u64 *out;
    const u64 *sk; // MUL: [.][N] NTT form, row i under prime i
    u64 seed, stream0, stream_step, item_stride;
    u64 n_polys; // items * polys
    int polys, logN;
    u64 lim[kMaxPrimes]; // bfv_seeded_limit(q_i)
};

template <bool MUL>
__global__ void __launch_bounds__(kBlock) k_bfv_seeded_gen(BfvSeededGenArgs A, const PrimeDev *primes)
{
    // a block lies inside one polynomial (N / 2 lanes of it, kBlock at a time): which one is block-uniform, 32-bit (the grid is below 2^31
    // blocks) and scalar work -- no lane divides
    static_assert(kBlock == 256, "a block owns 512 coefficients");
    const int bl = A.logN - 9; // log2 of the blocks per polynomial
    const u32 p = blockIdx.x >> bl;
    if (p >= A.n_polys) return;
    const u64 e2 = ((u64)(blockIdx.x & ((1u << bl) - 1)) << 8) | threadIdx.x;
    const u32 item = p / (u32)A.polys;
    const int i = (int)(p - item * (u32)A.polys);
    const ModU64 m = make_modu(primes[i]);
    const u64 lim = A.lim[i], base = bfv_seeded_base(A.seed, A.stream0 + item * A.stream_step + (u64)i);
    ulonglong2 v;
    v.x = bfv_seeded_uniform(base, 2 * e2, lim, m);
    v.y = bfv_seeded_uniform(base, 2 * e2 + 1, lim, m);
    if (MUL) {
        const ulonglong2 s = reinterpret_cast<const ulonglong2 *>(A.sk + ((u64)i << A.logN))[e2];
        v.x = barrett128((u128)v.x * s.x, m); v.y = barrett128((u128)v.y * s.y, m);
    }
    reinterpret_cast<ulonglong2 *>(A.out + item * A.item_stride + ((u64)i << A.logN))[e2] = v;
}

// w [n][L][N] coefficient form, plain [n][N] mod t or null -> c0 [n][L][N]
__global__ void __launch_bounds__(kBlock) k_bfv_seeded_finish(const u64 *w, const u64 *plain, u64 *c0, const PrimeDev *primes, BfvDeltaConst dc, u64 noise_seed,
                                                              u64 first_index, int L, int logN, u64 n_cts)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 r = gid >> (logN - 1), e2 = gid & (((u64)1 << (logN - 1)) - 1);
    if (r >= n_cts) return;
    const u64 base = bfv_seeded_base(noise_seed, client::seeded_e_stream(first_index + r));
    const int ex = bfv_seeded_error(base, 2 * e2), ey = bfv_seeded_error(base, 2 * e2 + 1);
    ulonglong2 m = make_ulonglong2(0, 0);
    u64 fx = 0, fy = 0;
    if (plain) {
        m = reinterpret_cast<const ulonglong2 *>(plain + (r << logN))[e2];
        fx = bfv_delta_fix(m.x, dc); fy = bfv_delta_fix(m.y, dc);
    }
    for (int i = 0; i < L; ++i) {
        const ModU64 mi = make_modu(primes[i]);
        const u64 at = (r * L + i) << logN;
        const ulonglong2 x = reinterpret_cast<const ulonglong2 *>(w + at)[e2];
        const u64 dx = plain ? bfv_delta_residue(m.x, fx, dc.qdivt[i], mi) : 0, dy = plain ? bfv_delta_residue(m.y, fy, dc.qdivt[i], mi) : 0;
        reinterpret_cast<ulonglong2 *>(c0 + at)[e2] = make_ulonglong2(bfv_seeded_finish(dx, ex, x.x, mi.q), bfv_seeded_finish(dy, ey, x.y, mi.q));
    }
}

__global__ void __launch_bounds__(kBlock) k_bfv_seeded_place(const u64 *c0, u64 *out, u32 n_polys /* n L */, int L, int logN)
{
    const int bl = logN - 9; // as k_bfv_seeded_gen: the residue polynomial (r, i) of a block is scalar work
    const u32 p = blockIdx.x >> bl;
    if (p >= n_polys) return;
    const u64 e2 = ((u64)(blockIdx.x & ((1u << bl) - 1)) << 8) | threadIdx.x;
    const u32 r = p / (u32)L, i = p - r * (u32)L;
    reinterpret_cast<ulonglong2 *>(out + (((u64)r * 2 * L + i) << logN))[e2] = reinterpret_cast<const ulonglong2 *>(c0 + ((u64)p << logN))[e2];
}

struct BfvSeededPlantArgs {
    const u64 *sel;
    u64 *c0;
    u64 n_polys; // n L residue polynomials
    u64 t, n_sel, first_slot;
    u64 inv_pow2[kMaxPrimes]; // (2^d)^(-1) mod q_i
    int L, logN;
    BfvDigitTab tab;
};
__global__ void __launch_bounds__(kBlock) k_bfv_seeded_plant(BfvSeededPlantArgs A, const PrimeDev *primes)
{
    const u64 gid = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 p = gid >> (A.logN - 1), e2 = gid & (((u64)1 << (A.logN - 1)) - 1);
    if (p >= A.n_polys) return;
    const u64 E = A.tab.total, lo = A.first_slot, hi = A.first_slot + A.n_sel * E; // the slots: coefficients lo .. hi - 1
    if (2 * e2 + 1 < lo || 2 * e2 >= hi) return;
    const u64 r = p / (u64)A.L;
    const int ii = (int)(p % (u64)A.L);
    const ModU64 mi = make_modu(primes[ii]);
    ulonglong2 *at = reinterpret_cast<ulonglong2 *>(A.c0 + (p << A.logN)) + e2;
    const ulonglong2 x = *at;
    u64 xs[2] = {x.x, x.y};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const u64 e = 2 * e2 + h;
        if (e < lo || e >= hi) continue;
        const u64 slot = e - lo, b = slot / E;
        const u32 d = (u32)(slot % E);
        if (bfv_digit_prime(A.tab, d) != ii) continue;
        xs[h] = addmod(xs[h], bfv_selector_value(A.sel[r * A.n_sel + b], A.t, (int)(d - A.tab.off[ii]), A.tab.w, A.inv_pow2[ii], mi), mi.q);
    }
    *at = make_ulonglong2(xs[0], xs[1]);
}

BfvSeededGenArgs gen_args(const KernelEnv &env, int polys, u64 items, u64 seed, u64 stream0, u64 stream_step, u64 *out, u64 item_stride, const u64 *sk)
{
    if (polys < 1 || polys > env.K) throw std::invalid_argument("seeded generation: more residue polynomials per item than the chain has primes");
    BfvSeededGenArgs A{};
    A.out = out; A.sk = sk; A.seed = seed; A.stream0 = stream0; A.stream_step = stream_step; A.item_stride = item_stride;
    A.n_polys = items * (u64)polys; A.polys = polys; A.logN = env.logn1 + kRowLog;
    for (int i = 0; i < polys; ++i) A.lim[i] = bfv_seeded_limit(env.prime_q[i]);
    return A;
}

} // namespace

void launch_bfv_seeded_gen(const KernelEnv &env, int polys, u64 items, u64 seed, u64 stream0, u64 stream_step, u64 *out, u64 item_stride, const u64 *sk)
{
    if (!items) return;
    const BfvSeededGenArgs A = gen_args(env, polys, items, seed, stream0, stream_step, out, item_stride, sk);
    const dim3 g(streaming_grid(A.n_polys, A.logN, "seeded generation")), b(kBlock);
    if (sk) hipLaunchKernelGGL(k_bfv_seeded_gen<true>, g, b, 0, env.stream, A, env.primes);
    else hipLaunchKernelGGL(k_bfv_seeded_gen<false>, g, b, 0, env.stream, A, env.primes);
}
void launch_bfv_seeded_finish(const KernelEnv &env, int L, u64 n, const u64 *w, const u64 *plain, const BfvDeltaConst &dc, u64 noise_seed, u64 first_index, u64 *c0)
{
    if (!n) return;
    if (L < 1 || L > env.Ltop) throw std::invalid_argument("he355_bfv_seeded_encrypt: level out of range");
    const int logN = env.logn1 + kRowLog;
    hipLaunchKernelGGL(k_bfv_seeded_finish, dim3(streaming_grid(n, logN, "he355_bfv_seeded_encrypt", "ciphertexts")), dim3(kBlock), 0, env.stream, w, plain, c0, env.primes,
                       dc, noise_seed, first_index, L, logN, n);
}
void launch_bfv_seeded_place(const KernelEnv &env, int L, u64 n, const u64 *c0, u64 *out)
{
    if (!n) return;
    const int logN = env.logn1 + kRowLog;
    const unsigned grid = streaming_grid(n * L, logN, "he355_bfv_seeded_restore"); // below 2^31 blocks: n L is a u32
    hipLaunchKernelGGL(k_bfv_seeded_place, dim3(grid), dim3(kBlock), 0, env.stream, c0, out, (u32)(n * L), L, logN);
}
void launch_bfv_seeded_plant(const KernelEnv &env, const BfvDigitTab &tab, int L, u64 n, u64 n_sel, u64 first_slot, int d, const u64 *sel, u64 t, u64 *c0)
{
    if (!n) return;
    if (L < 1 || L > kMaxPrimes || tab.L != L || !bfv_gadget_width_ok(tab.w) || d < 0 || d > env.logn1 + kRowLog ||
        first_slot + n_sel * tab.total > ((u64)1 << (env.logn1 + kRowLog)))
        throw std::invalid_argument("he355_bfv_seeded_selector_encrypt: level, digit table or slots out of range");
    BfvSeededPlantArgs A{};
    A.sel = sel; A.c0 = c0; A.n_polys = n * L; A.t = t; A.n_sel = n_sel; A.first_slot = first_slot;
    for (int i = 0; i < L; ++i) A.inv_pow2[i] = bfv_selector_inv_pow2(env.prime_q[i], d);
    A.L = L; A.logN = env.logn1 + kRowLog; A.tab = tab;
    hipLaunchKernelGGL(k_bfv_seeded_plant, dim3(streaming_grid(A.n_polys, A.logN, "he355_bfv_seeded_selector_encrypt")), dim3(kBlock), 0, env.stream, A, env.primes);
}

} // namespace HE355_KNS
} // namespace he355
