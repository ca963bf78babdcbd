// bfv_operands.inc -- BFV plaintext operands, modulus switching and NTT-form operands (he355_kernels_bfv_level.hip,
// he355_kernels_bfv_ntt.hip): launch sequences and C ABI together.  Included by he355_api.hip alone.  Every refusal of these calls is
// made after use(): the scheme check alone needs no device.

// Evaluator::add_plain / sub_plain (BFV): out = ct +- (Delta_L(plain), 0, ..); plain [.][N] mod t
static void bfv_addsub_plain(DeviceContext &d, int L, int size, u64 n, const u64 *ct, const u64 *plain, Indexer ix, u64 *out, bool sub)
{
    d.use();
    const Params &P = d.params();
    d.check_level(L);
    check_size(size, 1, 3);
    if (!n) return;
    const size_t N = P.N, ctn = (size_t)size * L * N;
    u64 a_lo, a_n, b_lo, b_n;
    d.indexer_span(ix, n, a_lo, a_n, b_lo, b_n);
    // in place exactly where every ciphertext serves one result (pairwise, or one plaintext per ciphertext): result r then reads what it writes
    const bool in_place = out == ct + a_lo * ctn && (ix.pairwise || ix.b1 == 1);
    if (!in_place && ranges_overlap(out, n * ctn, ct + a_lo * ctn, a_n * ctn)) throw std::invalid_argument("he355_bfv_add_plain / sub_plain: `out` overlaps the ciphertexts (in place only when each serves one result)");
    if (ranges_overlap(out, n * ctn, plain + b_lo * N, b_n * N)) throw std::invalid_argument("he355_bfv_add_plain / sub_plain: `out` overlaps the plaintexts");
    launch_bfv_addsub_plain(d.env(), L, size, n, ct, plain, ix, out, d.bfv_delta(L), sub);
    HIPCHECK(hipGetLastError());
}
// ---- NTT-form BFV operands (he355_kernels_bfv_ntt.hip) -------------------------------------------------------------------
// Evaluator::transform_to_ntt_inplace / transform_from_ntt_inplace of ciphertexts: [n][size][L][N], polynomial (k, i) under prime i.
// In place, or apart (copied, then transformed where it lands).  The library does not track which form a slab is in.
static void bfv_transform(DeviceContext &d, int L, int size, u64 n, const u64 *in, u64 *out, bool inverse)
{
    const char *what = inverse ? "he355_bfv_transform_from_ntt" : "he355_bfv_transform_to_ntt";
    d.use();
    const Params &P = d.params();
    d.check_level(L);
    check_size(size, 1, 3);
    const size_t N = P.N, words = (size_t)n * size * L * N;
    if (out != in && ranges_overlap(in, words, out, words)) throw std::invalid_argument(std::string(what) + ": `out` overlaps `in` (in place: the same pointer)");
    if (n * size > 0xffffffffull) throw std::invalid_argument(std::string(what) + ": too many polynomials for one call");
    if (!n) return;
    if (out != in) HIPCHECK(hipMemcpyAsync(out, in, words * 8, hipMemcpyDeviceToDevice, d.stream()));
    const PolyView v = d.poly_view(out, L, N, L);
    if (inverse) launch_ntt_inverse(d.env(), v, (u32)(n * size));
    else launch_ntt_forward(d.env(), v, (u32)(n * size));
    HIPCHECK(hipGetLastError());
}

extern "C" {
// Evaluator::mod_switch_to (BFV): [n][size][L][N] -> [n][size][L_to][N], L - L_to divide-and-round steps in one launch
int he355_bfv_mod_switch(he355_ctx *c, int L, int L_to, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_mod_switch");
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        d.check_level(L);
        if (L_to < 1 || L_to > L) throw std::invalid_argument("target level out of range");
        check_size(size, 1, 3);
        if (L > kBfvLevelMaxL) throw std::invalid_argument("BFV modulus switching supports up to 16 data primes");
        const size_t N = P.N, n_polys = (size_t)n * size;
        if (ranges_overlap(in, n_polys * L * N, out, n_polys * L_to * N)) throw std::invalid_argument("he355_bfv_mod_switch: `out` overlaps `in`");
        if (!n) return;
        if (L_to == L) {
            HIPCHECK(hipMemcpyAsync(out, in, n_polys * L * N * 8, hipMemcpyDeviceToDevice, d.stream()));
            return;
        }
        launch_bfv_mod_switch(d.env(), d.bfv_drop_table_dev(), (int)P.Ltop, L, L_to, n_polys, in, out);
        HIPCHECK(hipGetLastError());
    });
}
int he355_bfv_add_plain(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *pt, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { need_bfv(c, "he355_bfv_add_plain"); bfv_addsub_plain(dev(c), L, size, n, ct, pt, to_ix(ix), out, false); });
}
int he355_bfv_sub_plain(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *pt, he355_indexer ix, uint64_t *out)
{
    return guarded([&] { need_bfv(c, "he355_bfv_sub_plain"); bfv_addsub_plain(dev(c), L, size, n, ct, pt, to_ix(ix), out, true); });
}
// Evaluator::multiply_plain (BFV, multiply_plain_normal): every polynomial times the centred lift of the plaintext, negacyclic.
// Each distinct plaintext of the call is lifted and transformed once under the L primes (on stream(), ahead of the chunk loop: the
// fork event chunk 0 records orders the second stream behind it, and behind whatever produced the operands); a chunk is three
// launches -- forward column pass ct -> out, the fused row kernel in place on out, inverse column pass.
int he355_bfv_multiply_plain(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *plain, he355_indexer hix, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_multiply_plain");
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const Indexer ix = to_ix(hix);
        d.check_level(L);
        check_size(size, 1, 3);
        if (!n) return;
        const size_t N = P.N, LN = (size_t)L * N, ctn = (size_t)size * LN;
        u64 a_lo, a_n, b_lo, b_n;
        d.indexer_span(ix, n, a_lo, a_n, b_lo, b_n);
        if (ranges_overlap(out, n * ctn, ct + a_lo * ctn, a_n * ctn) || ranges_overlap(out, n * ctn, plain + b_lo * N, b_n * N))
            throw std::invalid_argument("he355_bfv_multiply_plain: `out` overlaps an operand");
        u64 *prep = d.bfv_arena(b_n * LN * 8);
        if (!prep) throw OutOfDeviceMemory("HIP error: out of device memory: the prepared plaintexts of he355_bfv_multiply_plain do not fit");
        d.plain_to_ntt(L, b_n, plain + b_lo * N, prep);
        d.for_each_chunk(n, L, d.chunk_ops(n, L, true), true, [&](u64 off, u64 nc, int which, const DeviceContext::Scratch &, hipEvent_t fork) {
            const KernelEnv env = d.batch_env(which);
            launch_bfv_mp_cols_fwd(env, L, size, nc, off, ct, ix, out);
            launch_bfv_mp_rows(env, L, size, nc, off, ct, prep, ix, out);
            launch_cols_inv(env, d.poly_view(out + off * ctn, size * L, N, L), (u32)nc);
            if (fork) HIPCHECK(hipEventRecord(fork, env.stream));
        });
        HIPCHECK(hipGetLastError());
    });
}
int he355_bfv_transform_to_ntt(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] { need_bfv(c, "he355_bfv_transform_to_ntt"); bfv_transform(dev(c), L, size, n, in, out, false); });
}
int he355_bfv_transform_from_ntt(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] { need_bfv(c, "he355_bfv_transform_from_ntt"); bfv_transform(dev(c), L, size, n, in, out, true); });
}
// Evaluator::transform_to_ntt_inplace(Plaintext, parms_id): plain [n][N] mod t -> out [n][L][N], the centred lift he355_bfv_multiply_plain
// multiplies by, transformed under primes 0 .. L-1
int he355_bfv_plain_to_ntt(he355_ctx *c, int L, uint64_t n, const uint64_t *plain, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_plain_to_ntt");
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        d.check_level(L);
        const size_t N = P.N;
        if (ranges_overlap(out, (size_t)n * L * N, plain, (size_t)n * N)) throw std::invalid_argument("he355_bfv_plain_to_ntt: `out` overlaps the plaintexts");
        if (n > 0xffffffffull) throw std::invalid_argument("he355_bfv_plain_to_ntt: too many plaintexts for one call");
        if (!n) return;
        d.plain_to_ntt(L, n, plain, out);
        HIPCHECK(hipGetLastError());
    });
}
// Evaluator::multiply_plain on NTT-form operands (multiply_plain_ntt): every polynomial times the NTT-form plaintext, k_plain_op's product
int he355_bfv_multiply_plain_ntt(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, const uint64_t *pt, he355_indexer hix, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_multiply_plain_ntt");
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const Indexer ix = to_ix(hix);
        d.check_level(L);
        check_size(size, 1, 3);
        if (!n) return;
        const size_t LN = (size_t)L * P.N, ctn = (size_t)size * LN;
        u64 a_lo, a_n, b_lo, b_n;
        d.indexer_span(ix, n, a_lo, a_n, b_lo, b_n);
        // in place exactly where every ciphertext serves one result: result r then reads the words it writes (as he355_bfv_add_plain)
        const bool in_place = out == ct + a_lo * ctn && (ix.pairwise || ix.b1 == 1);
        if (!in_place && ranges_overlap(out, n * ctn, ct + a_lo * ctn, a_n * ctn)) throw std::invalid_argument("he355_bfv_multiply_plain_ntt: `out` overlaps the ciphertexts (in place only when each serves one result)");
        if (ranges_overlap(out, n * ctn, pt + b_lo * LN, b_n * LN)) throw std::invalid_argument("he355_bfv_multiply_plain_ntt: `out` overlaps the plaintexts");
        launch_plain_op(d.env(), L, size, n, ct, pt, ix, out, 0);
        HIPCHECK(hipGetLastError());
    });
}
// out(i, j) = sum_k ct(i, k) (.) pt(k, j): the multiply_plain / add_inplace loop of a plaintext matrix x encrypted vector, one launch on
// the context's stream (nothing to fork: no scratch, no second stream)
int he355_bfv_multiply_plain_accumulate(he355_ctx *c, int L, int size, uint64_t rows, uint64_t cols, uint64_t inner, const uint64_t *ct, uint64_t ct_stride_i,
                                        uint64_t ct_stride_k, const uint64_t *pt, uint64_t pt_stride_k, uint64_t pt_stride_j, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_multiply_plain_accumulate");
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        d.check_level(L);
        check_size(size, 1, 3);
        if (inner < 1 || inner > 0x7fffffff) throw std::invalid_argument("inner dimension out of range");
        const u64 n = rows * cols;
        if (!n) return;
        const size_t LN = (size_t)L * P.N, ctn = (size_t)size * LN;
        const size_t n_ct = (size_t)((inner - 1) * ct_stride_k + (rows - 1) * ct_stride_i + 1), n_pt = (size_t)((inner - 1) * pt_stride_k + (cols - 1) * pt_stride_j + 1);
        if (ranges_overlap(out, n * ctn, ct, n_ct * ctn) || ranges_overlap(out, n * ctn, pt, n_pt * LN))
            throw std::invalid_argument("he355_bfv_multiply_plain_accumulate: `out` overlaps an operand");
        launch_bfv_plain_mac(d.env(), L, size, rows, cols, inner, ct, ct_stride_i, ct_stride_k, pt, pt_stride_k, pt_stride_j, out);
        HIPCHECK(hipGetLastError());
    });
}
} // extern "C"
