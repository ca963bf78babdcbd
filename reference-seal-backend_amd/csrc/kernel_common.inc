// kernel_common.inc -- helpers shared by the kernel translation units (every he355_kernels*.hip, one kernel family each):
// wavefront-scope hand-offs, engine construction, row <-> register moves, the LDS-DMA row fetch, the wave-level row transforms, the
// block's twiddle staging and, host side, the LOGN1 dispatch of every launcher with a per-ring instantiation and the grid sizes of the
// BFV PIR launches (dispatch_logn1, grid_blocks, streaming_grid).  Included INSIDE the anonymous namespace of a kernel file (after
// ntt_core.h), once per build of the u64 engine; the text is what one kernel file held in place through round 5 and the key-switch
// files shared until they were split (same token stream: tools/kres.py shows identical registers / spills / LDS for every instantiation).
// (kBlock, kWaves -- the block of the row kernels -- are ks_launch.h's, where the grids that assume them are computed)

// Each wave exchanges data only inside its own LDS region: LDS instructions of one wave execute in
// order, so a wavefront-scope release/acquire pair (compiler ordering only) is all the hand-off needs.
#define HE_WAVE_SYNC()                                             \
    do {                                                           \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     \
        __builtin_amdgcn_wave_barrier();                           \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");     \
    } while (0)

// Twiddle tables are reached through pointers stored in PrimeDev (HBM), which the compiler would treat as
// generic (flat_load + full s_waitcnt per access).  They are always global memory: say so.
__device__ __forceinline__ gtw_t gtw(const Tw16 *p) { return (gtw_t)p; }
__device__ __forceinline__ ctw_t ctw(const Tw16 *p) { return (ctw_t)(unsigned long long)p; } // lane-uniform entries: scalar loads

__device__ __forceinline__ ArU64 make_ar(const PrimeDev &p, ArU64 *)
{
    ArU64 a;
    a.q = p.q; a.two_q = p.q * 2; a.ninv = p.ninv; a.ninv_q = p.ninv_q; a.cr0 = p.cr0; a.cr1 = p.cr1;
    return a;
}
__device__ __forceinline__ ArF64 make_ar(const PrimeDev &p, ArF64 *)
{
    ArF64 a;
    a.q = p.qd; a.qinv = p.qinv; a.ninv = p.ninv_d; a.ninv_i = p.ninv_i;
    return a;
}
__device__ __forceinline__ ModU64 make_modu(const PrimeDev &p)
{
    ModU64 m;
    m.q = p.q; m.cr0 = p.cr0; m.cr1 = p.cr1;
    return m;
}

// ---- row <-> register moves ---------------------------------------------------------------------------
__device__ __forceinline__ void load_rowA(const u64 *row, int lane, u64 v[kRowE])
{
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = row[(r << 6) | lane];
}
__device__ __forceinline__ void store_rowA(u64 *row, int lane, const u64 v[kRowE])
{
#pragma unroll
    for (int r = 0; r < kRowE; ++r) row[(r << 6) | lane] = v[r];
}
// layout C (ntt_core.h elemC): registers 4c..4c+3 of a lane are 4 consecutive elements (32 bytes); the 4 lanes of a quad
// cover 128 consecutive bytes per chunk c, quads are 512 bytes apart
__device__ __forceinline__ void load_rowC(const u64 *row, int lane, u64 v[kRowE])
{
    const u64 *base = row + ((lane >> 2) << 6) + ((lane & 3) << 2);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const ulonglong2 *p = reinterpret_cast<const ulonglong2 *>(base + (c << 4));
        const ulonglong2 lo = p[0], hi = p[1];
        v[4 * c + 0] = lo.x; v[4 * c + 1] = lo.y; v[4 * c + 2] = hi.x; v[4 * c + 3] = hi.y;
    }
}
__device__ __forceinline__ void store_rowC(u64 *row, int lane, const u64 v[kRowE])
{
    u64 *base = row + ((lane >> 2) << 6) + ((lane & 3) << 2);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        ulonglong2 *p = reinterpret_cast<ulonglong2 *>(base + (c << 4));
        p[0] = make_ulonglong2(v[4 * c + 0], v[4 * c + 1]);
        p[1] = make_ulonglong2(v[4 * c + 2], v[4 * c + 3]);
    }
}

// ---- host side: launches of the kernels with a column pass, and grids ------------------------------------------------------------------
// launch(std::integral_constant<int, LOGN1>) for the ring's LOGN1 = logn1 in LO..5 (N = 2048 .. 32768; LO = 1: N = 1024 has no column
// pass; LO = 0: the kernels that take N = 1024 as a column of one).  A context has no other ring (Params: N in [1024, 32768]).
template <int LO = 1, class Launch>
void dispatch_logn1(int logn1, Launch &&launch)
{
    static_assert(LO == 0 || LO == 1, "the lowest ring is N = 1024 or N = 2048");
    switch (logn1 < LO ? -1 : logn1) {
    case 0:
        if constexpr (LO == 0) launch(std::integral_constant<int, 0>());
        break;
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 3: launch(std::integral_constant<int, 3>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 5: launch(std::integral_constant<int, 5>()); break;
    default: throw std::invalid_argument("ring size out of range");
    }
}
// a grid of `blocks` blocks, refused where it does not fit one launch ("<what>: too many <unit> for one launch").  `what` is a string
// literal; this and streaming_grid are templates only so that the kernel files that include this text and launch no such grid
// instantiate nothing (no unused-function warning, and no <string> asked of them).
template <class What>
unsigned grid_blocks(u64 blocks, What what, const char *unit = "polynomials")
{
    if (blocks > 0x7fffffffull) throw std::invalid_argument(std::string(what) + ": too many " + unit + " for one launch");
    return (unsigned)blocks;
}
// the grid of a streaming kernel whose lanes own two coefficients each: N / 2 is a multiple of kBlock, so a block lies inside one polynomial
template <class What>
unsigned streaming_grid(u64 n_polys, int logN, What what, const char *unit = "polynomials")
{
    return grid_blocks((n_polys << (logN - 1)) / kBlock, what, unit);
}

// Key products issued together in the fused fp64 k_k3 (2 polynomials x kMacG / 2 elements): interleaved chains, at two waves per
// SIMD a serial chain issues at 3/4 of the pipe's rate.
constexpr int kMacG = 4;

// ---- LDS-DMA: one 8 KiB row, HBM -> this wave's LDS staging buffer, no VGPRs, asynchronous -------------
// Each global_load_lds_dwordx4 moves 64 x 16 B; the LDS image is the row in natural element order.
// Completion is covered by the issuing wave's vmcnt (s_waitcnt vmcnt(0) before the first ds_read).
typedef __attribute__((address_space(3))) void lds_void_t;
// The instruction is issued from inline assembly, i.e. hidden from the compiler's wait-count insertion.
// Through the builtin (__builtin_amdgcn_global_load_lds), every ds_read that follows a DMA in program order gets an s_waitcnt vmcnt(0) in front of it whenever the
// compiler cannot rule out that it reads the landing buffer -- in k_k3 that is the first LDS exchange of the row transform, a third
// of the way into the step the DMA was meant to hide behind (ISA of round 2's kernel).  The kernels wait for a landing buffer
// themselves (asm volatile s_waitcnt vmcnt(0) before they read it); vector-memory results return in issue order, so the waits the
// compiler places for its own, younger loads stay sufficient.  M0 (LDS base of the DMA) is used by nothing else in these kernels.
template <int PIECES = 8> // 1 KiB pieces of the row slot that hold data (8: a row of 64-bit words; 6: a 48-bit packed digit row)
__device__ __forceinline__ void dma_row_to_lds(const u64 *grow, u64 *lds_row, int lane)
{
    const u32 lbase = __builtin_amdgcn_readfirstlane((u32)(unsigned long long)(lds_void_t *)lds_row);
    const u64 *g = grow + (lane << 1);
#pragma unroll
    for (int k = 0; k < PIECES; ++k)
        // non-temporal (round 5): a row is read once, by this wave -- served from L2 past the L1, which the block's eight waves share for the
        // key rows of the digit step (headline -0.7 %, configs[3] / [4] -1 %: profiles/r05_small_ab.txt)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt" ::"s"(lbase + (u32)(k << 10)), "v"(g + (k << 7)) : "memory");
}
__device__ __forceinline__ void lds_rowA(const u64 *lds_row, int lane, u64 v[kRowE])
{
#pragma unroll
    for (int r = 0; r < kRowE; ++r) v[r] = lds_row[(r << 6) | lane];
}

// ---- 48-bit digit rows (fp64-engine targets) -----------------------------------------------------------
// The digit slab is the largest HBM stream of a key switch (written once by k_k2, read once by k_k3) and the chip's mixed
// read/write bandwidth bounds the sequence, so a digit row of an fp64-engine prime is stored in 6 of the 8 KiB of its slot:
// a plane of 1024 low 32-bit words, then a plane of 1024 high 16-bit words, of the bit pattern of (x + kPackBias), x an
// integer with |x| < 2^47.  The pattern's top 16 bits are then always 0x4338, so 48 bits carry the value exactly.
constexpr double kPackBias = 4503599627370496.0 + 2251799813685248.0 + 140737488355328.0; // 2^52 + 2^51 + 2^47
constexpr int kPackHiOff = 4096;                                                          // byte offset of the high plane in the slot
__device__ __forceinline__ double unpack48(u32 lo, u32 hi16)
{
    union { u64 u; double d; } c;
    c.u = ((u64)(0x43380000u | hi16) << 32) | lo;
    return c.d - kPackBias;
}
__device__ __forceinline__ void lds_rowA48(const u64 *lds_row, int lane, double x[kRowE])
{
    const u32 *lo = reinterpret_cast<const u32 *>(lds_row);
    const unsigned short *hi = reinterpret_cast<const unsigned short *>(reinterpret_cast<const unsigned char *>(lds_row) + kPackHiOff);
#pragma unroll
    for (int r = 0; r < kRowE; ++r) x[r] = unpack48(lo[(r << 6) | lane], hi[(r << 6) | lane]);
}
// ---- wave-level row transforms (x in: layout A for forward, layout C for inverse) ---------------------
// lds_w: the wave's exchange buffer.  The twiddles of phase B / C are gathered BEFORE the exchange that precedes the phase and
// pinned there with a scheduling barrier, so their loads are in flight while the exchange round-trips through LDS.
struct NoHook {
    __device__ __forceinline__ void operator()() const {}
};
// `before_c` runs after phase B's math and before the second exchange: a caller uses it to put global loads in flight
// that it needs right after the transform (they then land during the exchange and phase C).
// LAZY (u64 engine, q < 2^60, rows entering below 4q): the wide lazy range of ntt_core.h's row_fwd_*_lazy -- results below 12q, for
// consumers that take any 64-bit lazy value (k_k3's key multiply-accumulate); ignored by the fp64 engine.
template <class Ar, class TW, class Hook = NoHook, bool LAZY = false>
__device__ __forceinline__ void wave_rows_fwd_n(const Ar &ar, const TW &tw, int lane, u64 *lds_w, typename Ar::T (*x)[kRowE], Hook before_c = Hook())
{
    typedef typename Ar::T T;
    T *lds = reinterpret_cast<T *>(lds_w);
    Tw16 wa[kTwA];
    gather_A(tw, wa);
    if constexpr (LAZY) row_fwd_A_lazy<1>(ar, x, wa); else row_fwd_A<1>(ar, x, wa);
    Tw16 wb[kTwB];
    gather_B(tw, lane, wb);
    __builtin_amdgcn_sched_barrier(0);
    lds_store_A(lds, lane, x[0]);
    HE_WAVE_SYNC();
    lds_load_B(lds, lane, x[0]);
    HE_WAVE_SYNC();
    if constexpr (LAZY) row_fwd_B_lazy<1>(ar, x, wb); else row_fwd_B<1>(ar, x, wb);
    Tw16 wc[kTwC];
    gather_C(tw, lane, wc);
    before_c();
    __builtin_amdgcn_sched_barrier(0);
    lds_store_B(lds, lane, x[0]);
    HE_WAVE_SYNC();
    lds_load_C(lds, lane, x[0]);
    HE_WAVE_SYNC();
    if constexpr (LAZY) row_fwd_C_lazy<1>(ar, x, wc); else row_fwd_C<1>(ar, x, wc);
}
template <class Ar, class TW>
__device__ __forceinline__ void wave_rows_fwd(const Ar &ar, const TW &tw, int lane, u64 *lds_w, typename Ar::T x[kRowE])
{
    wave_rows_fwd_n(ar, tw, lane, lds_w, reinterpret_cast<typename Ar::T(*)[kRowE]>(x));
}
// The inverse row pass on a row-local copy of the row's inverse twiddles (TwRow / TwRowF64, staged in LDS by the block: k_k1's
// throughput shape, where the four waves of a block work on the same (prime, row) of four ciphertexts): every phase's twiddles are
// LDS reads of this wave's own block instead of 46 scattered 16-byte loads per lane from the 512 KiB table in L2.
template <class Ar, class TW>
__device__ __forceinline__ void wave_rows_inv_tw(const Ar &ar, const TW &itw, const Tw16 &w0_scaled, bool last, int lane, u64 *lds_w, typename Ar::T x[kRowE])
{
    typedef typename Ar::T T;
    T *lds = reinterpret_cast<T *>(lds_w);
    row_inv_C(ar, x, itw, lane);
    Tw16 wb[kTwInvB];
    gather_inv_B(itw, lane, wb);
    __builtin_amdgcn_sched_barrier(0);
    lds_store_C(lds, lane, x);
    HE_WAVE_SYNC();
    lds_load_B(lds, lane, x);
    HE_WAVE_SYNC();
    row_inv_B_w(ar, x, wb);
    Tw16 wa[kTwInvA];
    gather_inv_A(itw, wa);
    __builtin_amdgcn_sched_barrier(0);
    lds_store_B(lds, lane, x);
    HE_WAVE_SYNC();
    lds_load_A(lds, lane, x);
    HE_WAVE_SYNC();
    if (last) row_inv_A_w<Ar, true>(ar, x, wa, w0_scaled);
    else row_inv_A_w<Ar, false>(ar, x, wa, w0_scaled);
}
template <class Ar>
__device__ __forceinline__ void wave_rows_inv(const Ar &ar, const PrimeDev &P, bool last, u32 rowbase, int lane, u64 *lds_w, typename Ar::T x[kRowE])
{
    typedef typename Ar::T T;
    T *lds = reinterpret_cast<T *>(lds_w);
    const auto itw = tw_table(gtw(P.inv), rowbase);
    row_inv_C(ar, x, itw, lane);
    // the twiddles of the next phase are requested before the exchange that precedes it (round 5; the forward pass always did): they land
    // while the exchange round-trips through LDS instead of behind it -- phase A's are lane-uniform, scalar loads
    Tw16 wb[kTwInvB];
    gather_inv_B(itw, lane, wb);
    __builtin_amdgcn_sched_barrier(0);
    lds_store_C(lds, lane, x);
    HE_WAVE_SYNC();
    lds_load_B(lds, lane, x);
    HE_WAVE_SYNC();
    row_inv_B_w(ar, x, wb);
    Tw16 wa[kTwInvA];
    gather_inv_A(tw_table(ctw(P.inv), rowbase), wa);
    __builtin_amdgcn_sched_barrier(0);
    lds_store_B(lds, lane, x);
    HE_WAVE_SYNC();
    lds_load_A(lds, lane, x);
    HE_WAVE_SYNC();
    if (last) row_inv_A_w<Ar, true>(ar, x, wa, P.inv_w0_scaled);
    else row_inv_A_w<Ar, false>(ar, x, wa, P.inv_w0_scaled);
}

// Stage the 1023 forward twiddles of row `rowbase` of prime P in LDS (one copy per block): every wave, digit and op
// of a (prime, row) tile reads them from there (ds_read, lane-dependent index) instead of L2.  fp64 engine: w only.
// The caller synchronises the block before the first use.
template <class Ar, int BLOCK>
__device__ __forceinline__ typename std::conditional<std::is_same<Ar, ArF64>::value, TwRowF64, TwRow>::type
stage_row_twiddles(const PrimeDev &P, const Ar &ar, u32 rowbase, unsigned char *twl_raw, bool inverse = false)
{
    constexpr bool kF64 = std::is_same<Ar, ArF64>::value;
    typename std::conditional<kF64, TwRowF64, TwRow>::type twr;
    const gtw_t gf = gtw(inverse ? P.inv : P.fwd); // (the two tables share their indexing: entry (rowbase << s) + g of stage s)
    constexpr int kIter = (kRowTw + BLOCK - 1) / BLOCK;
    Tw16 tmp[kIter];
#pragma unroll
    for (int k = 0; k < kIter; ++k) { // all loads in flight together
        const u32 i = threadIdx.x + k * BLOCK;
        tmp[k] = tw_load(gf, tw_row_source(rowbase, i + 1 < (u32)kRowTw ? i : 0));
    }
    if constexpr (kF64) {
        double *twl = reinterpret_cast<double *>(twl_raw);
#pragma unroll
        for (int k = 0; k < kIter; ++k)
            if (threadIdx.x + k * BLOCK < (u32)kRowTw) twl[threadIdx.x + k * BLOCK] = ArF64::tw_w(tmp[k]);
        twr.t = twl;
        twr.qinv = ar.qinv;
    } else {
        Tw16 *twl = reinterpret_cast<Tw16 *>(twl_raw);
#pragma unroll
        for (int k = 0; k < kIter; ++k)
            if (threadIdx.x + k * BLOCK < (u32)kRowTw) twl[threadIdx.x + k * BLOCK] = tmp[k];
        twr.t = twl;
    }
    return twr;
}
