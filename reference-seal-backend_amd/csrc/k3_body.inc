// Body of k_k3 (he355_kernels_k3.hip), textually included: once in the template kernel k_k3<Ar, WAVES, FUSE, TENSOR, GROUPED>
// (K3_BID_X / K3_BID_Y = blockIdx.x / blockIdx.y: the same token stream as before the split, hence the same code object -- the
// register allocation of the headline's instantiations is the product's bottleneck and a __device__ function boundary changed it,
// 48.5 -> 49.0 ms per step) and once per engine in k_k3_dual, the latency shape's both-engines-in-one-launch kernel.
// In scope at the point of inclusion: Ar, WAVES, FUSE, TENSOR, GROUPED, A (K3Args), primes; macros K3_BID_X, K3_BID_Y, K3_LDS_DECL.
    // TENSOR without FUSE is the rescale's divided-out prime (launch_k3, K3Fuse::raw_tail): the sums start from the operand rows and take the
    // fused instantiation's digit loop, but no correction rows and no floor step follow -- the sums leave through the inverse row pass of
    // the unfused epilogue, raw rows into A.tpr (k_floor_colsn<., true> subtracts the mod-down correction in coefficient form)
    static_assert(!GROUPED || !TENSOR, "grouped keys are for rotations");
    constexpr int kWaves = WAVES, kBlock = WAVES * 64; // this kernel's own block shape (shadows the file-wide one)
    typedef typename Ar::T T;
    typedef typename Ar::Acc Acc;
    constexpr bool kF64 = std::is_same<Ar, ArF64>::value;
    constexpr bool kPacked = kF64;                    // this engine's digit rows are 48-bit packed (k_k2n wrote them so)
    constexpr int kDigitPieces = kPacked ? 6 : 8;
    K3_LDS_DECL // lds[kWaves][kLdsRow], stage[kWaves][kRowN], twl_raw[]: the kernel's own __shared__ arrays, or the dual kernels' shared set
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 n1 = 1u << A.logn1;
    const u64 N = (u64)n1 << kRowLog;
    // XCD-aware mapping: blocks b and b+8 share an XCD (round-robin dispatch), so all op-groups of one
    // (tt,row) tile are placed on the same XCD back to back: its 2*L key rows stay in that XCD's L2.
    // A block stays on its tile for og_per_block consecutive op-groups (4 ops each): the twiddle staging and the block
    // start-up are paid once per og_per_block * 4 ops instead of once per 4.
    const u64 n_og = (A.n_ops + kWaves - 1) / kWaves;
    const u64 n_ogb = (n_og + A.og_per_block - 1) / A.og_per_block;
    const u64 total_tiles = (u64)A.n_tt * n1;
    const u64 s = K3_BID_X >> 3, xcd = K3_BID_X & 7;
    const u64 tile = (s / n_ogb) * 8 + xcd;
    if (tile >= total_tiles) return; // whole block exits together
    const u64 og_first = A.og_stride > 1 ? s % n_ogb : (s % n_ogb) * A.og_per_block;
    const int tt = A.tt_list[tile >> A.logn1];
    const int q_slot = A.q_slot[tile >> A.logn1];
    const u32 a_row = (u32)(tile & (n1 - 1));
    const int t = (tt == A.L) ? A.K - 1 : tt;
    const PrimeDev &P = primes[t];
    const Ar ar = make_ar(P, (Ar *)nullptr);
    const u64 rowoff = (u64)a_row << kRowLog;
    // this block's forward twiddles of row (t, a_row), staged once in LDS
    const auto twr = stage_row_twiddles<Ar, kBlock>(P, ar, n1 + a_row, twl_raw);
    __syncthreads();
    for (u32 g = 0; g < A.og_per_block; ++g) {
        const u64 og = og_first + (u64)g * A.og_stride;
        if (og >= n_og) break; // block-uniform
        u64 op = og * kWaves + wave;
        const bool valid = op < A.n_ops;
        if (!valid) op = A.n_ops - 1;
        Acc acc0[kRowE], acc1[kRowE];
#pragma unroll
        for (int r = 0; r < kRowE; ++r) { acc0[r] = 0; acc1[r] = 0; }
        auto tensor_init = [&](T c2[kRowE]) {
            if constexpr (TENSOR) {
                // ct x ct multiply: c0 = a0 b0 and c1 = a0 b1 + a1 b0 are not read back from k_k1's c01 rows, they start the sums -- here,
                // where no other row is live yet (the first digit row is on its way into LDS meanwhile).  The floor step computes
                // (sums - x) * P^-1 + addend (mod-down) or ((sums * P^-1 + addend) - x) * q_last^-1 (with the rescale); this instantiation is
                // handed key residues that carry the factor P^-1 already (DeviceContext::relin_scaled), so its sums ARE sums * P^-1 and the
                // addend joins them as it is: the results are sums' - x * P^-1 and (sums' - x) * q_last^-1 (floor_fin_s / floor_fin2_s), the
                // same residues exactly (modular identities), with two products per element fewer at this end and one fewer at that.
                // Three products from one load and one conversion of each operand row: c0 = a0 b0, c2 = a1 b1 (the digit that lives under
                // this prime, handed to the caller) and c1 = (a0 + a1)(b0 + b1) - c0 - c2, the same residue as a0 b1 + a1 b0 (dy_mul3).
                const u64 tr = A.t_op_offset + op;
                const u64 LNt = (u64)A.L * N;
                const u64 *pa = A.ta + idx_a(A.tix, tr) * 2 * LNt + (u64)tt * N + rowoff;
                const u64 *pb = A.tb + idx_b(A.tix, tr) * 2 * LNt + (u64)tt * N + rowoff;
                u64 a0[kRowE], a1[kRowE], b0[kRowE], b1[kRowE];
                load_rowC(pa, lane, a0); load_rowC(pb, lane, b0);
                load_rowC(pa + LNt, lane, a1); load_rowC(pb + LNt, lane, b1);
#pragma unroll
                for (int r = 0; r < kRowE; ++r) {
                    T p0, p1;
                    ar.dy_mul3(ar.dy_in(a0[r]), ar.dy_in(a1[r]), ar.dy_in(b0[r]), ar.dy_in(b1[r]), p0, p1, c2[r]);
                    acc0[r] = ar.acc_from_lazy(p0);
                    acc1[r] = ar.acc_from_lazy(p1);
                }
            }
        };
        // u64 engine: products added since the accumulators were last brought under 4q (wave-uniform); acc_flush before anything reads them
        constexpr int kRun = Ar::kAccRun;
        int pend = 0;
        auto acc_flush = [&]() {
            if constexpr (kRun > 1) {
                if (pend) {
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) { acc0[r] = ar.acc_reduce(acc0[r]); acc1[r] = ar.acc_reduce(acc1[r]); }
                    pend = 0;
                }
            }
        };
        auto acc_step = [&]() { // after one product went into every accumulator
            if constexpr (kRun > 1) {
                if (++pend == kRun) acc_flush();
            }
        };
        auto mac_row = [&](Acc acc[kRowE], const T x[kRowE], const u64 kv[kRowE], const u64 kq[kRowE]) {
#pragma unroll
            for (int r = 0; r < kRowE; ++r) {
                if constexpr (kRun > 1) ar.acc_mac_lazy(acc[r], x[r], ar.key_in(kv[r]), Ar::kKeyQuotient ? kq[r] : 0);
                else ar.acc_mac(acc[r], x[r], ar.key_in(kv[r]), Ar::kKeyQuotient ? kq[r] : 0);
            }
        };
        const u64 *kbase = A.key, *kqbase = A.keyq;
        if constexpr (GROUPED) { // this wave's op names its key (one scalar load per op)
            typedef const __attribute__((address_space(4))) unsigned long long *ckeys_t;
            const u32 grp = __builtin_amdgcn_readfirstlane((u32)((A.g_op_offset + op) / A.groups.group_size));
            kbase = (const u64 *)((ckeys_t)(unsigned long long)A.groups.key)[grp];
            kqbase = kbase + A.keyq_offset;
        }
        auto key_row = [&](int j, int k) -> const u64 * { return kbase + (((u64)j * 2 + k) * A.K + t) * N + rowoff; };
        auto keyq_row = [&](int j, int k) -> const u64 * { return kqbase + (((u64)j * 2 + k) * A.n_q + q_slot) * N + rowoff; };
        auto mac_poly = [&](Acc acc[kRowE], const T x[kRowE], int j, int k) {
            u64 kv[kRowE], kq[kRowE];
            load_rowC(key_row(j, k), lane, kv);
            if constexpr (Ar::kKeyQuotient) load_rowC(keyq_row(j, k), lane, kq);
            mac_row(acc, x, kv, kq);
        };
        auto mac_digit = [&](const T x[kRowE], int j) {
            mac_poly(acc0, x, j, 0);
            mac_poly(acc1, x, j, 1);
            acc_step();
        };
        // c1_mode 4 (a rotation without addend): row `rowoff` of polynomial `poly` of the Galois-permuted input, gathered from the input itself
        auto gather_base = [&](int poly, const uint32_t *&pm) -> const u64 * { // residue tt of polynomial `poly` of the op's source ciphertext; pm: this row's slice of the permutation
            u64 src_ct = A.gsrc_op_offset + op;
            pm = A.gperm;
            if constexpr (GROUPED) { // the op's group names its source block and its permutation table (as k_k1 reads them)
                const u32 gop = (u32)(A.g_op_offset + op), gi = __builtin_amdgcn_readfirstlane(gop / A.groups.group_size);
                src_ct = (u64)A.groups.src_block[gi] * A.groups.group_size + gop % A.groups.group_size;
                pm = A.groups.perm[gi];
            }
            pm += rowoff;
            return A.gsrc + (src_ct * 2 + (u64)poly) * ((u64)A.L * N) + (u64)tt * N;
        };
        auto gather_row = [&](int poly, u64 v[kRowE]) {
            const uint32_t *pm;
            const u64 *p0 = gather_base(poly, pm);
            // (read where they lie, sixteen 8-byte loads per lane: staging the source row in the exchange buffer, as k_k1 does, costs this kernel
            // 20-30 more spilled registers in its fused instantiations: configs[3] +4 %, configs[4] +0.5 %, profiles/r05_rotation_gather.txt)
#pragma unroll
            for (int r = 0; r < kRowE; ++r) v[r] = p0[pm[elemC(lane, r)]];
        };
        // digits that go through the forward row pass: all of them, except (CKKS) the one that lives under this very
        // prime -- that one is the NTT-form target itself and is multiplied in directly
        const bool has_own = A.ckks && tt < A.L;
        const int nd = A.L - (has_own ? 1 : 0);
        auto digit = [&](int i) -> int { return (has_own && i >= tt) ? i + 1 : i; };
        // this block's share of the transformed digits: all of them, or group K3_BID_Y of n_split (unfused instantiations only)
        const int split = FUSE ? 1 : (A.n_split > 1 ? A.n_split : 1), grp = split > 1 ? (int)K3_BID_Y : 0;
        const int i_begin = nd * grp / split, i_end = nd * (grp + 1) / split;
        auto src_row = [&](int j) -> const u64 * { return A.d + ((op * (A.L + 1) + tt) * A.L + j) * N + rowoff; };
        if (i_begin < i_end) dma_row_to_lds<kDigitPieces>(src_row(digit(i_begin)), stage[wave], lane);
        T c2[kRowE]; // TENSOR: a1 b1 out of tensor_init, dead again behind the own digit's key product (nothing else lives across it)
        tensor_init(c2);
        if (has_own && grp == 0) {
            if constexpr (TENSOR) {
                // the digit that lives under this prime is c2 = a1 b1 in NTT form (k_k1 writes no c2n row for a ct x ct multiply): the
                // product as tensor_init formed it (fp64 engine: centred lazy, |x| < q; the key product takes any |x k| < 2^100)
                mac_digit(c2, tt);
            } else {
                T x[kRowE];
                u64 v[kRowE];
                load_rowC(FUSE && A.c1_mode == 3 ? A.c1_src + (op * 3 + 2) * ((u64)A.L * N) + (u64)tt * N + rowoff : A.c2n + (op * A.L + tt) * N + rowoff, lane, v);
#pragma unroll
                for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(v[r]);
                mac_digit(x, tt);
            }
        }
        if constexpr (FUSE || TENSOR) {
            // One digit per wave, mod-down (and rescale) finished here.  The correction rows ride the same pipeline as the digit
            // rows: rows [0, nd) are digits (transform + key MAC), rows nd, nd+1 the special-prime correction of polynomial
            // 0 / 1 (transform, then (sums - x) * P^-1 + c01), rows nd+2, nd+3 the rescale correction (transform, then
            // (result - x) * q_last^-1).  Every row is prefetched into the LDS landing buffer behind the previous row's math.
            // resc: the rescale is finished here too.  Its correction slab already holds delta2 + P^-1 * delta1 (k_floor_cols folded
            // the mod-down correction in), so there are two correction rows per tile either way:
            //   mod-down only: rows nd, nd+1 from cols:   c01 <- (sums - x) * P^-1 + c01
            //   with rescale : rows nd, nd+1 from cols2:  out <- ((sums * P^-1 + c01) - x) * q_last^-1
            const bool resc = A.cols2 != nullptr;
            const int n_rows = nd + 2;
            const u64 LN = (u64)A.L * N, L1N = (u64)(A.L - 1) * N;
            auto row_ptr = [&](int i) -> const u64 * {
                if (i < nd) return src_row(digit(i));
                if (!resc) return A.cols + ((op * 2 + (i - nd)) * A.L + tt) * N + rowoff;
                return A.cols2 + ((op * 2 + (i - nd)) * (A.L - 1) + tt) * N + rowoff;
            };
            const FloorConst fc = A.fc[(A.K - 1) * A.K + t];
            const FloorConst fc2 = A.fc[(resc ? A.L - 1 : 0) * A.K + t];
            if (FUSE && nd == 0) dma_row_to_lds(row_ptr(0), stage[wave], lane); // no digit row was primed above
            // digit rows: transform + key MAC (the last one prefetches the first correction row)
            for (int i = 0; i < nd; ++i) {
                T x[1][kRowE];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this step's row has landed in LDS
                if constexpr (kPacked) {
                    lds_rowA48(stage[wave], lane, x[0]);
                } else {
                    u64 v[kRowE];
                    lds_rowA(stage[wave], lane, v);
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) x[0][r] = ar.from_raw(v[r]);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // staging buffer drained into registers
                // next row, behind this step's math: a digit row (packed for this engine) or the first correction row (64-bit words)
                if (i + 1 < nd) dma_row_to_lds<kDigitPieces>(row_ptr(i + 1), stage[wave], lane);
                else if constexpr (FUSE) dma_row_to_lds(row_ptr(i + 1), stage[wave], lane);
                if constexpr (!Ar::kKeyQuotient) {
                    // both key rows of the digit are requested before the second exchange (the hook runs after phase B's math): they
                    // land behind the exchange and phase C instead of in front of the multiply-accumulate, which used to wait out
                    // two L2 round trips per step (poly 0, then poly 1)
                    u64 kv0[kRowE], kv1[kRowE];
                    const int j = digit(i);
                    wave_rows_fwd_n(ar, twr, lane, lds[wave], x, [&]() { load_rowC(key_row(j, 0), lane, kv0); load_rowC(key_row(j, 1), lane, kv1); });
                    // the 32 products, kMacG at a time (interleaved chains: at two waves per SIMD a serial chain issues at 3/4 of the
                    // pipe's rate)
                    if constexpr (kF64) {
#pragma unroll
                        for (int r0 = 0; r0 < kRowE; r0 += kMacG / 2) {
                            double xs[kMacG], ks[kMacG], pr[kMacG];
#pragma unroll
                            for (int k = 0; k < kMacG / 2; ++k) {
                                xs[2 * k] = x[0][r0 + k]; ks[2 * k] = ar.key_in(kv0[r0 + k]);
                                xs[2 * k + 1] = x[0][r0 + k]; ks[2 * k + 1] = ar.key_in(kv1[r0 + k]);
                            }
                            ar.template mulmod_vv_g<kMacG>(xs, ks, pr);
#pragma unroll
                            for (int k = 0; k < kMacG / 2; ++k) { acc0[r0 + k] += pr[2 * k]; acc1[r0 + k] += pr[2 * k + 1]; }
                        }
                    }
                } else { // u64 engine: the digit rows are transformed over the wide lazy range (one correction per row, not per butterfly)
                    wave_rows_fwd_n<Ar, decltype(twr), NoHook, true>(ar, twr, lane, lds[wave], x);
                    mac_digit(x[0], digit(i));
                }
            }
            acc_flush();
            // fp64 engine: the floor steps read the double sums as they are (no canonical integer in between).  Where this prime's bound
            // does not hold for the launch's number of terms (at most L digits and the operand products: three centred terms in c1 =
            // (a0 + a1)(b0 + b1) - a0 b0 - a1 b1 of a ct x ct multiply, kTensorTerms; modarith.h, floor_direct_terms) sums and correction
            // row are re-centred first -- one wave-uniform branch per row.
            // (Read here, behind the digit loop: one more value live across it costs the rotation instantiations spilled registers.)
            // kAccForms: the plain rotation / size-3 instantiation <FUSE, !TENSOR, !GROUPED> keeps the canonical forms -- with the accumulator
            // forms its allocation changes (34 -> 58 spilled registers on the fp64 engine, one reload inside the digit step, whose
            // s_waitcnt also waits for the prefetched row: DotProduct 38.9 -> 41.1 ms per step), the other instantiations' improves.
            constexpr bool kAccForms = TENSOR || GROUPED;
            const bool direct = kAccForms && Ar::kAccDirect && floor_direct(P.acc_terms, (u32)A.L + (TENSOR ? kTensorTerms : 2u));
            // correction rows: transform + floor step(s)
#pragma unroll 1
            for (int i = nd; FUSE && i < n_rows; ++i) {
                T x[1][kRowE];
                u64 v[kRowE], av[kRowE];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                lds_rowA(stage[wave], lane, v);
#pragma unroll
                for (int r = 0; r < kRowE; ++r) x[0][r] = ar.from_raw(v[r]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (i + 1 < n_rows) dma_row_to_lds(row_ptr(i + 1), stage[wave], lane);
                const int k = i - nd;
                u64 *c01_row = A.c01 + op * A.c01_item_stride + k * LN + (u64)tt * N + rowoff;
                // the addend, in flight during the transform -- or nothing: for a ct x ct multiply (A.ta) it entered the accumulators before the digits
                if constexpr (TENSOR) {
                    // (no addend row: it entered the sums before the digits)
                } else if (k == 0 && A.c1_mode == 4) { // a rotation without addend, polynomial 0: the permuted c0, gathered from the input
                    gather_row(0, av);
                } else if (k == 0 && A.c1_mode == 5) { // a rotation WITH addend, polynomial 0: addend0 + the permuted c0 (k_k1 neither added nor wrote them)
                    u64 ad[kRowE];
                    load_rowC(A.c1_src + (op * 2 + 0) * LN + (u64)tt * N + rowoff, lane, ad);
                    gather_row(0, av);
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) av[r] = addmod(av[r], ad[r], P.q);
                } else if (k == 1 && (A.c1_mode == 1 || A.c1_mode == 4)) { // a rotation without addend: polynomial 1 starts from zero (k_k1 wrote no row of zeros)
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) av[r] = 0;
                } else if (A.c1_mode == 3) { // relinearize of a size-3 ciphertext: c0, c1 read from the input itself (k_k1 copied nothing)
                    load_rowC(A.c1_src + (op * 3 + k) * LN + (u64)tt * N + rowoff, lane, av);
                } else { // ... with addend: its polynomial 1, read where it lies
                    load_rowC(k == 1 && (A.c1_mode == 2 || A.c1_mode == 5) ? A.c1_src + (op * 2 + 1) * LN + (u64)tt * N + rowoff : c01_row, lane, av);
                }
                // level sum (KsGroups::sum_out), a node one step ends at and nothing starts from -- most of a level: its ciphertext is wanted
                // only inside the sum, so the sum's row joins the ADDEND of the floor step and the result is the sum's new row (one load
                // beside the addend's, no second pass over the row)
                bool into_sum = false;
                u64 *sum_row = nullptr;
                u32 sum_cnt = 0;
                if constexpr (GROUPED && !TENSOR) {
                    if (A.groups.sum_out) {
                        const u32 gop = (u32)(A.g_op_offset + op), gi = __builtin_amdgcn_readfirstlane(gop / A.groups.group_size);
                        sum_cnt = A.groups.count[gi];
                        sum_row = A.groups.sum_out + ((u64)(gop % A.groups.group_size) * 2 + k) * LN + (u64)tt * N + rowoff;
                        into_sum = sum_cnt == 1 && !resc;
                        if (into_sum) {
                            u64 o[kRowE];
                            load_rowC(sum_row, lane, o);
#pragma unroll
                            for (int r = 0; r < kRowE; ++r) av[r] = addmod(av[r], o[r], P.q);
                        }
                    }
                }
                if constexpr (!kF64 && Ar::kFold) {
                    // fold build of the u64 engine: the correction rows take the wide lazy pass too (below 8q + 16c), one lazy_reduce
                    // (three instructions per element) puts them under the 4q the floor steps read
                    wave_rows_fwd_n<Ar, decltype(twr), NoHook, true>(ar, twr, lane, lds[wave], x);
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) x[0][r] = ar.lazy_reduce(x[0][r]);
                } else {
                    wave_rows_fwd_n(ar, twr, lane, lds[wave], x);
                }
                const Acc *acc = k == 0 ? acc0 : acc1;
                if (kAccForms && Ar::kAccDirect && !direct) { // beyond the direct forms' bound: sums (not read again after this row) and row re-centred
                    if (k == 0) {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) ar.floor_prep(acc0[r], x[0][r]);
                    } else {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) ar.floor_prep(acc1[r], x[0][r]);
                    }
                }
                if constexpr (TENSOR) { // sums formed with scaled key residues, addend inside them
                    if (!resc) {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) v[r] = ar.floor_fin_s_acc(acc[r], x[0][r], fc.inv, fc.inv_shoup, fc.inv_d, fc.inv_i);
                        if (valid) store_rowC(c01_row, lane, v);
                    } else {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) v[r] = ar.floor_fin2_s_acc(acc[r], x[0][r], fc2);
                        if (valid) store_rowC(A.out2 + (op * 2 + k) * L1N + (u64)tt * N + rowoff, lane, v);
                    }
                } else if (!resc) {
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) {
                        if constexpr (kAccForms) v[r] = ar.floor_fin_acc(acc[r], x[0][r], fc.inv, fc.inv_shoup, fc.inv_d, fc.inv_i, av[r]);
                        else v[r] = ar.floor_fin(ar.acc_canon(acc[r]), x[0][r], fc.inv, fc.inv_shoup, fc.inv_d, fc.inv_i, av[r]);
                    }
                    if constexpr (GROUPED) {
                        if (into_sum) {
                            if (valid) store_rowC(sum_row, lane, v);
                        } else if (A.groups.sum_out) {
                            // the other nodes of a level sum: this wave alone touches row (ciphertext, k, tt, row) of the sum during the launch,
                            // group after group in program order; the group's own ciphertext is kept only for the next level to start from
                            if (valid && (sum_cnt & kGroupKeepBit)) store_rowC(c01_row, lane, v);
                            const u32 m = sum_cnt & ~kGroupKeepBit;
                            if (m) {
                                u64 o[kRowE];
                                load_rowC(sum_row, lane, o);
                                for (u32 rep = 0; rep < m; ++rep)
#pragma unroll
                                    for (int r = 0; r < kRowE; ++r) o[r] = addmod(o[r], v[r], P.q);
                                if (valid) store_rowC(sum_row, lane, o);
                            }
                        } else if (valid) store_rowC(c01_row, lane, v);
                    } else if (valid) store_rowC(c01_row, lane, v);
                } else {
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) {
                        if constexpr (kAccForms) v[r] = ar.floor_fin2_acc(acc[r], x[0][r], fc, fc2, av[r]);
                        else v[r] = ar.floor_fin2(ar.acc_canon(acc[r]), x[0][r], fc, fc2, av[r]);
                    }
                    if (valid) store_rowC(A.out2 + (op * 2 + k) * L1N + (u64)tt * N + rowoff, lane, v);
                }
            }
        }
        if constexpr (!FUSE) {
            for (int i = i_begin; !TENSOR && i < i_end; ++i) {
                T x[1][kRowE];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this step's row has landed in the staging buffer
                if constexpr (kPacked) {
                    lds_rowA48(stage[wave], lane, x[0]);
                } else {
                    u64 v[kRowE];
                    lds_rowA(stage[wave], lane, v);
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) x[0][r] = ar.from_raw(v[r]);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // staging buffer drained into registers
                if (i + 1 < i_end) dma_row_to_lds<kDigitPieces>(src_row(digit(i + 1)), stage[wave], lane); // next step's row, behind this step's math
                wave_rows_fwd_n<Ar, decltype(twr), NoHook, true>(ar, twr, lane, lds[wave], x);
                mac_digit(x[0], digit(i));
            }
            acc_flush();
            // Epilogue: canonical sums, NTT form, layout C.  Data primes -> t; special prime -> tp.  Where the next step is the
            // inverse transform of these very rows (the special prime always; every prime for BFV, whose key switch returns to
            // coefficient form) the wave runs the inverse row pass right here and writes the raw rows (special prime -> tpr).
            const bool inv_here = TENSOR || tt == A.L || !A.ckks;
            const bool last = A.logn1 == 0;
            // (the raw-tail form: polynomial 1's sums wait in the wave's landing buffer -- no row is on its way into it any more, and
            // each lane reads back only what it wrote -- so that the first inverse pass does not run with 32 more live registers than the
            // digit loop was allocated for.  The sums go into the inverse pass in the engine's cheapest form its first stage accepts
            // (acc_to_inv: the fp64 engine re-centres, no canonical integer in between); a TENSOR launch is never split and always
            // inverts here.)
            if constexpr (TENSOR) {
#pragma unroll
                for (int r = 0; r < kRowE; ++r) stage[wave][(r << 6) | lane] = ar.acc_park(acc1[r]);
            }
#pragma unroll 1
            for (int k = 0; k < 2; ++k) {
                u64 v[kRowE];
                T x[kRowE];
                if constexpr (TENSOR) {
                    if (k == 0) {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) x[r] = ar.acc_to_inv(acc0[r]);
                    } else {
#pragma unroll
                        for (int r = 0; r < kRowE; ++r) x[r] = ar.acc_unpark(stage[wave][(r << 6) | lane]);
                    }
                } else {
                    const Acc *acc = k == 0 ? acc0 : acc1;
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) v[r] = ar.acc_canon(acc[r]);
                    if (split > 1) { // a partial sum: k_k3_combine finishes the tile
                        if (valid) store_rowC(A.part + (((u64)grp * A.n_ops * 2 + op * 2 + k) * (A.L + 1) + tt) * N + rowoff, lane, v);
                        continue;
                    }
                    if (!inv_here) {
                        if (valid) store_rowC(A.t + ((op * 2 + k) * A.L + tt) * N + rowoff, lane, v);
                        continue;
                    }
#pragma unroll
                    for (int r = 0; r < kRowE; ++r) x[r] = ar.from_canon(v[r]);
                }
                wave_rows_inv(ar, P, last, n1 + a_row, lane, lds[wave], x);
#pragma unroll
                for (int r = 0; r < kRowE; ++r) v[r] = last ? ar.to_canon(x[r]) : ar.to_raw(x[r]);
                u64 *dst = tt < A.L && !TENSOR ? A.t + ((op * 2 + k) * A.L + tt) * N + rowoff : A.tpr + (op * 2 + k) * N + rowoff;
                if (valid) store_rowA(dst, lane, v);
            }
        }
    }
