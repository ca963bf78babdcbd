// Body of k_k2n (he355_kernels_ks.hip), textually included: in the template kernel k_k2n<LOGN1, WIDE> (K2N_BID_X = blockIdx.x: the token
// stream, and with it the code object of the headline's instantiations, is what it was before the split) and, behind a function
// boundary, once per digit kind in k_k2n_dual (latency shape).  In scope at the point of inclusion: LOGN1, WIDE, A (K2Args), primes.
    constexpr int N1 = 1 << LOGN1;
    constexpr u64 N = (u64)N1 << kRowLog;
    const u64 oj = K2N_BID_X >> 2;
    const u32 cb = K2N_BID_X & 3;
    const int col = (int)(cb << 8) | threadIdx.x;
    const u32 oj32 = (u32)oj; // n_ops * L < 2^32
    const int j = A.dig_list[__builtin_amdgcn_readfirstlane(oj32 % (u32)A.n_dig)];
    const u64 op = __builtin_amdgcn_readfirstlane(oj32 / (u32)A.n_dig);
    const u64 *src = A.c2r + op * A.src_op_stride + (u64)j * N;
    const PrimeDev &Pj = primes[j];
    const bool coeff_in = A.src_is_coeff || LOGN1 == 0; // BFV: coefficient form already; N = 1024: the row pass was the whole inverse
    constexpr bool kTile = N1 >= 8;
    __shared__ __attribute__((aligned(16))) unsigned char tiles[kTile ? kWaves : 1][kTile ? N1 * 384 : 16];
    unsigned char *tile = tiles[kTile ? threadIdx.x >> 6 : 0];
    if constexpr (WIDE) { // 60-bit digits: integers
        u64 c[N1];
        if (coeff_in) {
#pragma unroll
            for (int a = 0; a < N1; ++a) c[a] = src[(a << kRowLog) + col];
        } else {
            const ArU64 ar = make_ar(Pj, (ArU64 *)nullptr);
            u64 x[N1];
#pragma unroll
            for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
            col_inv<ArU64, LOGN1>(ar, x, ctw(Pj.inv), Pj.inv_w0_scaled);
#pragma unroll
            for (int a = 0; a < N1; ++a) c[a] = ar.to_canon(x[a]);
        }
        k2n_targets_f64<LOGN1, false>(A, primes, Pj, j, op, c, col, tile);
        k2n_targets_u64<LOGN1>(A, primes, Pj, j, op, c, col);
    } else {
    double c[N1];
    if (coeff_in) {
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = u52_to_f64(src[(a << kRowLog) + col]);
    } else if (Pj.f64) {
        const ArF64 ar = make_ar(Pj, (ArF64 *)nullptr);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.from_raw(src[(a << kRowLog) + col]);
        col_inv<ArF64, LOGN1>(ar, c, ctw(Pj.inv), Pj.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = ar.canon(c[a]);
    } else { // a u64-engine prime below 2^52
        const ArU64 ar = make_ar(Pj, (ArU64 *)nullptr);
        u64 x[N1];
#pragma unroll
        for (int a = 0; a < N1; ++a) x[a] = src[(a << kRowLog) + col];
        col_inv<ArU64, LOGN1>(ar, x, ctw(Pj.inv), Pj.inv_w0_scaled);
#pragma unroll
        for (int a = 0; a < N1; ++a) c[a] = u52_to_f64(ar.to_canon(x[a]));
    }
    k2n_targets_f64<LOGN1, true>(A, primes, Pj, j, op, c, col, tile);
    u64 cu[N1]; // the fp64 targets are done: the column continues as integers (the doubles die here)
#pragma unroll
    for (int a = 0; a < N1; ++a) cu[a] = f64_to_u52(c[a]);
    k2n_targets_u64<LOGN1>(A, primes, Pj, j, op, cu, col);
    }
