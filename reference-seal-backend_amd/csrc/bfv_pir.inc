// bfv_pir.inc -- the BFV PIR family: monomial multiply, query expansion and merging, digit decomposition, the gadget cuts, RGSW
// encryption, external product, selection tree and selectors, packed bytes, reply compression, seeded queries -- launch sequences and
// C ABI together.  Included by he355_api.hip alone.  The argument checks that need no device are bfv_pir_args.h's: every call makes them,
// and its plan, before it asks for one.

// ROUTED: a block of the column pass walks all E_i L digit columns of its residue one after the other, so a batch of fewer blocks than
// kGadgetColsMinBlocks (one per CU) leaves most of the chip idle and lost to the composition where it was measured (one ciphertext:
// profiles/bfv_external_product.txt); such a batch takes N = 1024's path, whose work is spread over the digit polynomials.
static constexpr u64 kGadgetColsMinBlocks = 256;
// does a cut of `cts` ciphertexts of `size` polynomials take the column pass?
static bool gadget_cols(const DeviceContext &d, u64 cts, int size, int L) { return d.env().logn1 != 0 && cts * size * L * 4 >= kGadgetColsMinBlocks; }
// the cut of ciphertext (a, b) at index a stride_a + b stride_b into NTT-form digit polynomials [(a n_b + b) size E + f][L][N]: N >= 2048 the
// fused column pass and the row pass in place, N = 1024 the digits under every prime and the whole transform in place.  No scratch.
static void gadget_cut_ntt(DeviceContext &d, const BfvDigitTab &tab, int L, int size, u64 n_a, u64 n_b, const u64 *ct, u64 stride_a, u64 stride_b, u64 *out)
{
    const Params &P = d.params();
    const u32 items = (u32)(n_a * n_b * size * tab.total);
    const bool cols = gadget_cols(d, n_a * n_b, size, L);
    ++(cols ? d.counters().routes.cut_cols : d.counters().routes.cut_stream);
    launch_bfv_gadget_cut(d.env(), tab, L, size, n_a, n_b, ct, stride_a, stride_b, out, cols);
    d.forward_rows_or_full(cols, d.poly_view(out, L, P.N, L), items);
}
// `rows` encryptions of zero, he355_encrypt_zero(seed, first_index + row), for a plant kernel that cuts them to the first L primes: made
// in `out` itself at L == L_top (the kernel then works in place, the block returned is empty), below it in the pool block returned
static PoolBlock zeros_at_level(DeviceContext &d, int L, u64 rows, u64 seed, u64 first_index, u64 *out)
{
    const Params &P = d.params();
    PoolBlock hold = (size_t)L < P.Ltop ? d.scoped_block((size_t)rows * 2 * P.Ltop * P.N * 8) : PoolBlock();
    d.encrypt(rows, nullptr, seed, first_index, hold ? hold.get() : out);
    return hold;
}
// plain [n][N] mod t -> out [n][2E][2][L][N] NTT form: row f of RGSW r is he355_encrypt_zero(seed, first_index + r 2E + f) cut to the first L
// primes, plus the planted term.
static void bfv_rgsw_encrypt(DeviceContext &d, const BfvRgswPlan &pl, int L, u64 n, const u64 *plain, u64 seed, u64 first_index, u64 *out)
{
    d.use();
    const Params &P = d.params();
    if (!n) return;
    if (!d.public_key()) throw std::invalid_argument("he355_bfv_rgsw_encrypt: public key not set");
    const PoolBlock hold = zeros_at_level(d, L, pl.rows, seed, first_index, out);
    const u64 *zero = hold ? hold.get() : out;
    launch_bfv_rgsw_plant(d.env(), pl.tab, L, (int)P.Ltop, n, zero, plain, P.plain_modulus, out);
    launch_ntt_forward(d.env(), d.poly_view(out, L, P.N, L), (u32)(pl.rows * 2));
    HIPCHECK(hipGetLastError());
}
// ---- seeded queries and Galois keys (he355_kernels_bfv_seeded.hip; the definition: bfv_seeded_core.h, include/he355.h) ----------------
// The seeded zero of index first_index + r, built at level L where it will lie: c0 = -e - iNTT(a (.) s), plus Delta_L(m).  Three launches
// whatever n is, all in place on `c0` (no scratch, so nothing to chunk): a (.) s generated straight into it, the inverse transform, the finish.
static void seeded_c0(DeviceContext &d, const char *what, int L, u64 n, const u64 *plain, u64 a_seed, u64 noise_seed, u64 first_index, u64 *c0)
{
    const Params &P = d.params();
    if (!d.secret_key()) throw std::invalid_argument(std::string(what) + ": secret key not set (he355_set_secret_key)");
    if (!n) return;
    const size_t N = P.N;
    launch_bfv_seeded_gen(d.env(), L, n, a_seed, client::seeded_a_stream(first_index, 0), 64, c0, (u64)L * N, d.secret_key());
    launch_ntt_inverse(d.env(), d.poly_view(c0, L, N, L), (u32)n);
    launch_bfv_seeded_finish(d.env(), L, n, c0, plain, d.bfv_delta(L), noise_seed, first_index, c0);
}

extern "C" {
// ---- monomial multiply and oblivious query expansion (he355_kernels_bfv_expand.hip) -------------------------------------------
// out = in X^e for every polynomial of [n][size][L][N], coefficient form: one launch
int he355_bfv_multiply_monomial(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *in, uint32_t e, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_multiply_monomial");
        check_monomial_args(*c->params, L, size, e);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t words = (size_t)n * size * L * P.N;
        if (ranges_overlap(in, words, out, words)) throw std::invalid_argument("he355_bfv_multiply_monomial: `out` overlaps `in`");
        launch_bfv_shift(d.env(), L, n * size * L, in, nullptr, e, out);
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_bfv_expand_galois_elts(const he355_ctx *c, uint64_t count, uint32_t *out, uint64_t cap)
{
    if (!c || c->params->scheme != kSchemeBFV || count < 1 || count > c->params->N) return 0;
    const int d = expand_depth(count);
    for (int j = 0; j < d && (uint64_t)j < cap; ++j) out[j] = (uint32_t)(c->params->N >> j) + 1;
    return (uint64_t)d;
}
// Oblivious expansion (Angel et al., "PIR with compressed queries", Alg. 3): in [n][2][L][N] -> out [count][n][2][L][N], child k of query r
// at index k n + r.  Level j (s = 2^j) turns the s n nodes it reads, node k of query r at k n + r, into 2 s n: ONE batched key switch
// with the node itself as the addend leaves the even children c + g where the nodes' indices are (k_bfv_galois forms c0 + sigma(c0) and
// passes c1 through, k_bfv_tail_fin adds the switched part; the addend is only read, so it may be the input), and one k_bfv_shift
// launch writes the odd children X^(-s) (2c - even) behind them, at (k + s) n + r -- the last level only those below `count`.  The
// levels alternate between `out` and one pool block of 2^(d-1) n ciphertexts (what level d - 2 writes), the parity chosen so that
// level d - 1 lands in `out`; everything runs on the context's stream.  Every refusal comes before the first launch.
int he355_bfv_expand(he355_ctx *c, int L, uint64_t n, const uint64_t *in, uint64_t count, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_expand");
        const BfvExpandPlan pl = plan_expand(*c->params, L, count);
        DeviceContext &dv = dev(c);
        dv.use();
        const Params &P = dv.params();
        const int d = pl.depth;
        const size_t N = P.N, ctn = 2 * (size_t)L * N;
        if (d) dv.require_keyswitch();
        for (int j = 0; j < d; ++j) {
            const uint32_t elt = (uint32_t)(N >> j) + 1;
            if (!dv.galois_key(elt)) throw std::invalid_argument("he355_bfv_expand: Galois key of element " + std::to_string(elt) + " not present");
        }
        if (ranges_overlap(in, n * ctn, out, count * n * ctn)) throw std::invalid_argument("he355_bfv_expand: `out` overlaps `in`");
        if (!n) return;
        if (!d) {
            HIPCHECK(hipMemcpyAsync(out, in, n * ctn * 8, hipMemcpyDeviceToDevice, dv.stream()));
            return;
        }
        const PoolBlock tmp = d > 1 ? dv.scoped_block(((size_t)n << (d - 1)) * ctn * 8) : PoolBlock();
        const u64 *cur = in;
        for (int j = 0; j < d; ++j) {
            const u64 s = (u64)1 << j, odd = std::min<u64>(s, count - s); // (count - s < s at the last level only)
            u64 *dst = (d - 1 - j) % 2 == 0 ? out : tmp.get();
            dv.apply_galois(L, s * n, cur, (uint32_t)(N >> j) + 1, dst, cur);
            launch_bfv_shift(dv.env(), L, odd * n * 2 * L, cur, dst, (u32)(2 * N - s), dst + s * n * ctn);
            cur = dst;
        }
        HIPCHECK(hipGetLastError());
    });
}
// The expansion's transpose (Chen, Dai, Kim, Song, "Efficient homomorphic conversion between (ring) LWE ciphertexts", Alg. 2): input k of
// result r at ciphertext k stride_k + r stride_r of `in` -> out [n][2][L][N].  Level j = d-1 .. 0 (s = 2^j) is ONE k_bfv_merge launch over the
// s n pairs of all results, pair k n + r, which leaves S = even + X^s odd and D = even - X^s odd (S = D = even where slot k + s is absent:
// the first level only) in two slabs, and ONE batched key switch of D with S as its addend, which leaves slot k of result r at k n + r:
// only the first level reads through the strides.  One pool block holds S, D and the level's output, each 2^(d-1) n ciphertexts, the first
// level's sizes (the later levels use the head of each; a level's output is consumed by the next merge launch before the next key switch
// writes there); the last level lands in `out`.  Everything runs on the context's stream; every refusal, the block's included, comes
// before the first launch.
int he355_bfv_merge(he355_ctx *c, int L, uint64_t n, uint64_t count, const uint64_t *in, uint64_t stride_k, uint64_t stride_r, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_merge");
        const BfvMergePlan pl = plan_merge(*c->params, L, n, count, in, stride_k, stride_r, out);
        DeviceContext &dv = dev(c);
        dv.use();
        const Params &P = dv.params();
        const int d = pl.depth;
        const size_t N = P.N, ctn = 2 * (size_t)L * N;
        if (d) dv.require_keyswitch();
        for (int j = d - 1; j >= 0; --j) {
            const uint32_t elt = (uint32_t)(N >> j) + 1;
            if (!dv.galois_key(elt)) throw std::invalid_argument("he355_bfv_merge: Galois key of element " + std::to_string(elt) + " not present");
        }
        if (!n) return;
        if (!d) { // count == 1: result r is its one input
            if (stride_r == 1 || n == 1) HIPCHECK(hipMemcpyAsync(out, in, n * ctn * 8, hipMemcpyDeviceToDevice, dv.stream()));
            else
                for (u64 r = 0; r < n; ++r) HIPCHECK(hipMemcpyAsync(out + r * ctn, in + r * stride_r * ctn, ctn * 8, hipMemcpyDeviceToDevice, dv.stream()));
            return;
        }
        const PoolBlock blk = dv.scoped_block((size_t)pl.scratch_cts * ctn * 8);
        u64 *S = blk.get(), *D = S + pl.half * ctn, *mid = D + pl.half * ctn; // mid: unused (and not there) when d == 1
        const u64 *cur = in;
        u64 have = count; // slots present
        for (int j = d - 1; j >= 0; --j) {
            const u64 s = (u64)1 << j;
            launch_bfv_merge(dv.env(), L, n, s, (have - s) * n, cur, stride_k, stride_r, S, D);
            u64 *dst = j ? mid : out;
            dv.apply_galois(L, s * n, D, (uint32_t)(N >> j) + 1, dst, S);
            cur = dst; stride_k = n; stride_r = 1; have = s;
        }
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_bfv_digit_count(const he355_ctx *c, int L, uint32_t *per_prime, uint64_t cap)
{
    if (!c || c->params->scheme != kSchemeBFV || L < 1 || (size_t)L > c->params->Ltop || c->params->plain_modulus < 2) return 0;
    const BfvDigitTab tab = digit_table(*c->params, L);
    for (int i = 0; i < L && (uint64_t)i < cap; ++i) per_prime[i] = tab.D[i];
    return tab.total;
}
// ---- ciphertext decomposition for recursive (two-dimensional) PIR (he355_kernels_bfv_digits.hip) ---------------------------------
// [n][size][L][N] -> [n][F][N] coefficients mod t: one streaming launch
int he355_bfv_decompose(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, uint64_t *plain)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_decompose");
        const BfvDigitPlan pl = plan_digits(*c->params, "he355_bfv_decompose", L, size, n, ct, plain);
        DeviceContext &d = dev(c);
        d.use();
        launch_bfv_digits(d.env(), pl.tab, L, size, n, ct, plain);
        HIPCHECK(hipGetLastError());
    });
}
// [n][size][L][N] -> [n][F][L_out][N], by definition bfv_decompose + bfv_plain_to_ntt(L_out, n F).  N >= 2048: the fused column pass
// reads the ciphertext, cuts, lifts and writes out(f, i'), the row pass runs in place -- no scratch.  N = 1024 has no column pass and is
// routed to the composition, its [n][F][N] slab a pool block (a second identical call allocates nothing).
int he355_bfv_decompose_ntt(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *ct, int L_out, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_decompose_ntt");
        const BfvDigitPlan pl = plan_digits(*c->params, "he355_bfv_decompose_ntt", L, size, n, ct, out, true, L_out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t N = P.N, F = pl.F;
        if (!n) return;
        if (d.env().logn1 == 0) {
            ++d.counters().routes.digits_routed;
            const PoolBlock tmp = d.scoped_block((size_t)n * F * N * 8);
            launch_bfv_digits(d.env(), pl.tab, L, size, n, ct, tmp.get());
            d.plain_to_ntt(L_out, n * F, tmp.get(), out);
            HIPCHECK(hipGetLastError());
            return;
        }
        ++d.counters().routes.digits_fused;
        launch_bfv_digits_cols_fwd(d.env(), pl.tab, L, size, n, ct, L_out, P.plain_modulus, out);
        launch_rows_fwd(d.env(), d.poly_view(out, L_out, N, L_out), (u32)(n * F));
        HIPCHECK(hipGetLastError());
    });
}
// the inverse: [n][F][N] -> [n][size][L][N], canonical whatever the digits are
int he355_bfv_compose(he355_ctx *c, int L, int size, uint64_t n, const uint64_t *plain, uint64_t *ct)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_compose");
        const BfvDigitPlan pl = plan_digits(*c->params, "he355_bfv_compose", L, size, n, ct, plain);
        DeviceContext &d = dev(c);
        d.use();
        launch_bfv_undigits(d.env(), pl.tab, L, size, n, plain, ct);
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_bfv_gadget_count(const he355_ctx *c, int L, int digit_bits, uint32_t *per_prime, uint64_t cap)
{
    if (!c || c->params->scheme != kSchemeBFV || L < 1 || (size_t)L > c->params->Ltop || !bfv_gadget_width_ok(digit_bits)) return 0;
    const BfvDigitTab tab = bfv_gadget_table(level_primes(*c->params, L).data(), L, digit_bits);
    for (int i = 0; i < L && (uint64_t)i < cap; ++i) per_prime[i] = tab.D[i];
    return tab.total;
}
// ---- the external product RGSW x ciphertext (he355_kernels_bfv_gadget.hip; the definition: bfv_gadget_core.h, include/he355.h) ----------
// [n][size][L][N] -> [n][size E][N], the plain integer digits of width v: he355_bfv_decompose's launch with the width-v table
int he355_bfv_gadget_decompose(he355_ctx *c, int L, int digit_bits, int size, uint64_t n, const uint64_t *ct, uint64_t *digits)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_gadget_decompose");
        const BfvDigitPlan pl = plan_gadget_cut(*c->params, "he355_bfv_gadget_decompose", L, digit_bits, size, n, ct, digits, false);
        DeviceContext &d = dev(c);
        d.use();
        launch_bfv_digits(d.env(), pl.tab, L, size, n, ct, digits);
        HIPCHECK(hipGetLastError());
    });
}
// [n][size][L][N] -> [n][size E][L][N]: by definition bfv_gadget_decompose, then he355_ntt_forward of every digit polynomial under every prime
int he355_bfv_gadget_decompose_ntt(he355_ctx *c, int L, int digit_bits, int size, uint64_t n, const uint64_t *ct, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_gadget_decompose_ntt");
        const BfvDigitPlan pl = plan_gadget_cut(*c->params, "he355_bfv_gadget_decompose_ntt", L, digit_bits, size, n, ct, out, true);
        DeviceContext &d = dev(c);
        d.use();
        if (!n) return;
        gadget_cut_ntt(d, pl.tab, L, size, n, 1, ct, 1, 0, out);
        HIPCHECK(hipGetLastError());
    });
}
int he355_bfv_rgsw_encrypt(he355_ctx *c, int L, int digit_bits, uint64_t n, const uint64_t *d_plain, uint64_t seed, uint64_t first_index, uint64_t *d_rgsw)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_rgsw_encrypt");
        const BfvRgswPlan pl = plan_rgsw(*c->params, L, digit_bits, n, d_plain, d_rgsw);
        bfv_rgsw_encrypt(dev(c), pl, L, n, d_plain, seed, first_index, d_rgsw);
    });
}
// ---- RGSW selectors from ONE packed query ciphertext (he355_kernels_bfv_gadget.hip; the definition: bfv_gadget_core.h, include/he355.h) -------
// sel [n][n_sel] mod t -> out [n][2][L][N], coefficient form: he355_encrypt_zero(seed, first_index + r) cut to the first L primes plus the planted
// selectors.
int he355_bfv_selector_encrypt(he355_ctx *c, int L, int digit_bits, uint64_t n, uint64_t n_sel, uint64_t first_slot, uint64_t count, const uint64_t *sel, uint64_t seed,
                               uint64_t first_index, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_selector_encrypt");
        const BfvSelectorPlan pl = plan_selector(*c->params, L, digit_bits, n, n_sel, first_slot, count, sel, out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!n) return;
        if (!d.public_key()) throw std::invalid_argument("he355_bfv_selector_encrypt: public key not set");
        const PoolBlock hold = zeros_at_level(d, L, n, seed, first_index, out);
        const u64 *zero = hold ? hold.get() : out;
        launch_bfv_selector_plant(d.env(), pl.tab, L, (int)P.Ltop, n, n_sel, first_slot, pl.depth, zero, sel, P.plain_modulus, out);
        HIPCHECK(hipGetLastError());
    });
}
// RGSW(s) at (L, key_bits): by definition bfv_rgsw_encrypt of the secret key's coefficients mod t (0, 1, t - 1).  The context holds s in NTT
// form: prime 0's residue goes through the inverse transform in one pool block of N words and is mapped there; the block is held across
// the inner call, whose plan (n = 1) is made here, once the plaintext has its address.
int he355_bfv_rgsw_encrypt_secret(he355_ctx *c, int L, int kv, uint64_t seed, uint64_t first_index, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_rgsw_encrypt_secret");
        check_rgsw_secret_args(*c->params, L, kv);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!d.secret_key()) throw std::invalid_argument("he355_bfv_rgsw_encrypt_secret: secret key not set");
        if (!d.public_key()) throw std::invalid_argument("he355_bfv_rgsw_encrypt_secret: public key not set");
        const size_t N = P.N;
        const PoolBlock s = d.scoped_block(N * 8);
        HIPCHECK(hipMemcpyAsync(s.get(), d.secret_key(), N * 8, hipMemcpyDeviceToDevice, d.stream()));
        launch_ntt_inverse(d.env(), d.poly_view(s.get(), 1, N, 1), 1);
        launch_bfv_secret_plain(d.env(), s.get(), P.plain_modulus);
        HIPCHECK(hipGetLastError());
        bfv_rgsw_encrypt(d, plan_rgsw(P, L, kv, 1, s.get(), out), L, 1, s.get(), seed, first_index, out);
    });
}
// out [n][n_sel][2E][2][L][N], NTT form.  Slot ciphertext c = (r n_sel + b) E + f (coefficient form, read where it lies): row f of RGSW (r, b) is its
// forward transform, row E + f the NTT-form sums of its key_bits digits against RGSW(s) -- what he355_bfv_external_product leaves before its
// inverse transform, which he355_bfv_transform_to_ntt would only undo.  A pass of slot ciphertexts (bfv_gadget_pass over the key's 2 E_key
// terms, one pool block as in bfv_external_product) is the cut, which also emits the slot's own column (gadget_cut_ntt's route, decided once per
// call from the first pass: every pass must leave the k = 0 rows in the same state), the digits' row pass and one multiply-accumulate into the
// k = 1 rows.  One row pass over the k = 0 rows, in place, ends the call.
int he355_bfv_rgsw_from_bfv(he355_ctx *c, int L, int digit_bits, int key_bits, uint64_t n, uint64_t n_sel, const uint64_t *ct, uint64_t ct_stride_r, uint64_t ct_stride_k,
                            const uint64_t *key, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_rgsw_from_bfv");
        const BfvFromBfvPlan pl = plan_from_bfv(*c->params, L, digit_bits, key_bits, n, n_sel, ct, ct_stride_r, ct_stride_k, key, out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!n) return;
        const size_t N = P.N, LN = (size_t)L * N;
        const u32 E = pl.tab.total, rows = pl.rows;
        const u64 C = pl.C, pass = pl.pass;
        const bool cols = gadget_cols(d, std::min<u64>(pass, C), 2, L);
        const PoolBlock slab = d.scoped_block((size_t)pass * rows * LN * 8);
        for (u64 c0 = 0; c0 < C; c0 += pass) {
            const u64 cnt = std::min<u64>(pass, C - c0);
            ++d.counters().routes.passes;
            ++(cols ? d.counters().routes.own_cols : d.counters().routes.own_stream);
            launch_bfv_gadget_cut_own(d.env(), pl.ktab, L, n_sel * E, c0, cnt, ct, ct_stride_r, ct_stride_k, slab.get(), out, E, cols);
            d.forward_rows_or_full(cols, d.poly_view(slab.get(), L, N, L), (u32)(cnt * rows));
            launch_bfv_gadget_mac_own(d.env(), L, c0, cnt, rows, slab.get(), key, out, E);
        }
        // the k = 0 rows: rows f0 .. f0 + R - 1 of every RGSW ciphertext are one item of R 2L polynomials, the items 2E 2L polynomials apart
        const u32 R = std::max<u32>(1, 64 / (2 * (u32)L));
        for (u32 f0 = 0; f0 < E; f0 += R) {
            PolyView pv = d.poly_view(out + (size_t)f0 * 2 * LN, (int)(std::min<u32>(R, E - f0) * 2 * L), N, L);
            pv.item_stride = (u64)2 * E * 2 * LN;
            d.forward_rows_or_full(cols, pv, (u32)(n * n_sel));
        }
        HIPCHECK(hipGetLastError());
    });
}
// ---- the selection tree (he355_kernels_bfv_gadget.hip; the definition: include/he355.h) ---------------------------------------------------
// out(r) = the fold of result r's `count` leaves under its depth RGSW bits: level j turns the c_j nodes of every result into c_(j+1), node'(p) =
// node(2p) + RGSW(r, j) [.] (node(2p+1) - node(2p)), the node without a partner copied.  Nodes lie result-major, [n][c_j]: level 0 reads
// the caller's leaves through its strides, the later levels alternate between the two halves of one pool block, the last one lands in `out`.
// A level is a pass loop over all pairs of all results (pl.pass of them per trip through the second pool block: 2E digit polynomials per
// pair and, behind them, the pass's sums -- at N = 1024 the level's): the DIFF cut (bfv_external_product's route rule for that many results), its row pass, one
// multiply-accumulate (k_bfv_plain_mac where the level has exactly one pair) into the sums, the inverse row pass in place and the
// inverse column pass that adds the even node and stores the next level's node.  N = 1024 has no column pass: ROUTED to
// launch_ntt_inverse and a streaming add.  One copy launch per level moves the nodes without a partner.  Both blocks are taken before the
// first launch; everything runs on the context's stream.
int he355_bfv_select(he355_ctx *c, int L, int digit_bits, uint64_t n, uint64_t count, const uint64_t *ct, uint64_t ct_stride_r, uint64_t ct_stride_k, const uint64_t *rgsw,
                     uint64_t rg_stride_r, uint64_t rg_stride_j, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_select");
        const BfvSelectPlan pl = plan_select(*c->params, L, digit_bits, n, count, ct, ct_stride_r, ct_stride_k, rgsw, rg_stride_r, rg_stride_j, out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!n) return;
        const size_t N = P.N, LN = (size_t)L * N, ctn = 2 * LN;
        const int m = pl.depth;
        if (!m) { // count == 1: result r is its one leaf
            launch_bfv_select_copy(d.env(), L, n, 0, ct, ct_stride_r, ct_stride_k, out, 1);
            HIPCHECK(hipGetLastError());
            return;
        }
        const u32 rows = pl.rows;
        const PoolBlock nodes = pl.node_cts ? d.scoped_block((size_t)pl.node_cts * ctn * 8) : PoolBlock();
        const PoolBlock slab = d.scoped_block((size_t)pl.slab_polys * N * 8);
        u64 *half[2] = {nodes ? nodes.get() : nullptr, nodes ? nodes.get() + n * pl.c[1] * ctn : nullptr};
        u64 *sums = slab.get() + pl.pass * rows * LN;
        // N = 1024: the sums of a whole LEVEL lie behind the digits and the routed tail runs once per level, not per pass -- the ring is
        // launch-bound, and per pass the two extra launches lost to the composition at 16 passes (profiles/bfv_select.txt, part 2b)
        const bool level_tail = d.env().logn1 == 0;
        const u64 *cur = ct;
        u64 stride_a = ct_stride_r, stride_b = ct_stride_k;
        for (int j = 0; j < m; ++j) {
            const u64 group = pl.c[j] / 2, pairs = pl.pairs(j), c_next = pl.c[j + 1];
            u64 *dst = j == m - 1 ? out : half[j & 1];
            const u64 *rg = rgsw + (size_t)j * rg_stride_j * rows * ctn;
            for (u64 p0 = 0; p0 < pairs; p0 += pl.pass) {
                const u64 cnt = std::min<u64>(pl.pass, pairs - p0);
                const bool cols = gadget_cols(d, cnt, 2, L);
                u64 *psum = sums + (level_tail ? p0 * ctn : 0);
                ++d.counters().routes.passes;
                ++(cols ? d.counters().routes.select_cols : d.counters().routes.select_stream);
                launch_bfv_select_cut(d.env(), pl.tab, L, group, p0, cnt, cur, stride_a, stride_b, slab.get(), cols);
                d.forward_rows_or_full(cols, d.poly_view(slab.get(), L, N, L), (u32)(cnt * rows));
                // ROUTED as bfv_external_product routes one result: a level of exactly one pair is k_bfv_plain_mac's 1 x 1 form
                const bool plain = pairs == 1;
                ++(plain ? d.counters().routes.mac_plain : d.counters().routes.mac_gadget);
                if (plain) launch_bfv_plain_mac(d.env(), L, 2, 1, 1, rows, rg, 1, 1, slab.get(), 1, 1, psum);
                else launch_bfv_select_mac(d.env(), L, group, p0, cnt, rows, slab.get(), rg, rg_stride_r, psum);
                if (level_tail) continue;
                launch_rows_inv(d.env(), d.poly_view(sums, L, N, L), (u32)(cnt * 2));
                launch_bfv_select_tail(d.env(), L, group, p0, cnt, sums, cur, stride_a, stride_b, dst, c_next);
            }
            if (level_tail) {
                launch_ntt_inverse(d.env(), d.poly_view(sums, L, N, L), (u32)(pairs * 2));
                launch_bfv_select_tail(d.env(), L, group, 0, pairs, sums, cur, stride_a, stride_b, dst, c_next);
            }
            ++(level_tail ? d.counters().routes.select_tail_routed : d.counters().routes.select_tail_fused);
            if (pl.c[j] & 1) launch_bfv_select_copy(d.env(), L, n, group, cur, stride_a, stride_b, dst, c_next);
            cur = dst; stride_a = c_next; stride_b = 1;
        }
        HIPCHECK(hipGetLastError());
    });
}
// out(r) = sum_kappa rgsw(r, kappa) [.] ct(r, kappa), coefficient form in and out.  By definition bfv_gadget_decompose_ntt of the inner
// ciphertexts of each result, he355_bfv_multiply_plain_accumulate(L, 2, 1, 1, inner 2E) with the RGSW rows as the ciphertext operand, and
// he355_bfv_transform_from_ntt.  The digit slab of a pass of results (bfv_gadget_pass: about kGadgetPassPolys digit polynomials, at least
// one result) is one pool block; a pass is the cut, its row pass and one batched multiply-accumulate; one inverse transform ends the call.
int he355_bfv_external_product(he355_ctx *c, int L, int digit_bits, uint64_t n, uint64_t inner, const uint64_t *ct, uint64_t ct_stride_r, uint64_t ct_stride_k,
                               const uint64_t *rgsw, uint64_t rg_stride_r, uint64_t rg_stride_k, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_external_product");
        const BfvExternalPlan pl = plan_external_product(*c->params, L, digit_bits, n, inner, ct, ct_stride_r, ct_stride_k, rgsw, rg_stride_r, rg_stride_k, out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!n) return;
        const size_t N = P.N, LN = (size_t)L * N;
        const u32 rows = pl.rows;
        const u64 terms = pl.terms, pass = pl.pass;
        const PoolBlock slab = d.scoped_block((size_t)pass * terms * LN * 8);
        for (u64 r0 = 0; r0 < n; r0 += pass) {
            const u64 cnt = std::min<u64>(pass, n - r0);
            gadget_cut_ntt(d, pl.tab, L, 2, cnt, inner, ct + r0 * ct_stride_r * 2 * LN, ct_stride_r, ct_stride_k, slab.get());
            const u64 *rg = rgsw + r0 * rg_stride_r * rows * 2 * LN;
            // ROUTED: a call for ONE result whose RGSW rows follow one another is the composition's own inner product, and
            // k_bfv_plain_mac's 1 x 1 form (two terms' loads in flight) measured 2-17 % ahead of k_bfv_gadget_mac there
            // (profiles/bfv_external_product.txt).  Only n == 1 was measured, so only n == 1 is routed: a pass that holds one result
            // of many (inner 2E above 2048, or a ragged last pass) stays with k_bfv_gadget_mac.
            const bool plain = n == 1 && (inner == 1 || rg_stride_k == 1);
            ++d.counters().routes.passes;
            ++(plain ? d.counters().routes.mac_plain : d.counters().routes.mac_gadget);
            if (plain) launch_bfv_plain_mac(d.env(), L, 2, 1, 1, terms, rg, 1, 1, slab.get(), 1, 1, out + r0 * 2 * LN);
            else launch_bfv_gadget_mac(d.env(), L, cnt, inner, rows, slab.get(), rg, rg_stride_r, rg_stride_k, out + r0 * 2 * LN);
        }
        launch_ntt_inverse(d.env(), d.poly_view(out, L, N, L), (u32)(n * 2));
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_bfv_bytes_per_plain(const he355_ctx *c, uint32_t *field_bits)
{
    if (!c || c->params->scheme != kSchemeBFV || c->params->plain_modulus < 2) return 0;
    const int w = bfv_bitlen(c->params->plain_modulus) - 1;
    if (field_bits) *field_bits = (uint32_t)w;
    return bfv_bytes_max(c->params->N, w);
}
// ---- a PIR database from packed bytes (he355_kernels_bfv_bytes.hip; the definition: bfv_bytes_core.h, include/he355.h) ----------------
// bytes -> [n][N] coefficients mod t: one streaming launch
int he355_bfv_unpack_bytes(he355_ctx *c, uint64_t n, const void *bytes, uint64_t stride, uint64_t B, uint64_t *plain)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_unpack_bytes");
        const BfvBytesPlan pl = plan_bytes(*c->params, "he355_bfv_unpack_bytes", n, bytes, stride, B, plain, false);
        DeviceContext &d = dev(c);
        d.use();
        launch_bfv_unpack(d.env(), pl.w, n, bytes, stride, B, plain);
        HIPCHECK(hipGetLastError());
    });
}
// bytes -> [n][L_out][N], by definition bfv_unpack_bytes + bfv_plain_to_ntt(L_out, n).  N >= 2048: the fused column pass reads the bytes,
// cuts, lifts and writes out(j, i'), the row pass runs in place -- no scratch.  N = 1024 has no column pass and is routed to the
// composition, kBytesChunk plaintexts at a time through one pool block (a database is large; a second identical call allocates nothing).
int he355_bfv_unpack_bytes_ntt(he355_ctx *c, int L_out, uint64_t n, const void *bytes, uint64_t stride, uint64_t B, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_unpack_bytes_ntt");
        const BfvBytesPlan pl = plan_bytes(*c->params, "he355_bfv_unpack_bytes_ntt", n, bytes, stride, B, out, false, true, L_out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t N = P.N;
        if (!n) return;
        if (d.env().logn1 == 0) {
            const u64 chunk = n < kBytesChunk ? n : kBytesChunk;
            const PoolBlock tmp = d.scoped_block((size_t)chunk * N * 8);
            for (u64 j = 0; j < n; j += chunk) {
                const u64 cnt = n - j < chunk ? n - j : chunk;
                ++d.counters().routes.bytes_routed;
                launch_bfv_unpack(d.env(), pl.w, cnt, static_cast<const unsigned char *>(bytes) + j * stride, stride, B, tmp.get());
                d.plain_to_ntt(L_out, cnt, tmp.get(), out + (size_t)j * L_out * N);
            }
            HIPCHECK(hipGetLastError());
            return;
        }
        ++d.counters().routes.bytes_fused;
        launch_bfv_bytes_cols_fwd(d.env(), pl.w, n, bytes, stride, B, L_out, P.plain_modulus, out);
        launch_rows_fwd(d.env(), d.poly_view(out, L_out, N, L_out), (u32)n);
        HIPCHECK(hipGetLastError());
    });
}
// the inverse: [n][N] words, each masked to w bits -> ceil(B / 8) whole words per plaintext
int he355_bfv_pack_bytes(he355_ctx *c, uint64_t n, const uint64_t *plain, uint64_t B, uint64_t stride, void *bytes)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_pack_bytes");
        const BfvBytesPlan pl = plan_bytes(*c->params, "he355_bfv_pack_bytes", n, bytes, stride, B, plain, true);
        DeviceContext &d = dev(c);
        d.use();
        launch_bfv_pack(d.env(), pl.w, n, plain, B, stride, bytes);
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_bfv_reply_bytes(const he355_ctx *c, int k0, int k1)
{
    if (!c || c->params->scheme != kSchemeBFV || !bfv_reply_widths_ok(c->params->N, c->params->primes[0].q, k0, k1)) return 0;
    return bfv_reply_size(c->params->N, k0, k1);
}
int he355_bfv_reply_safe_bits(const he355_ctx *c, int *k0, int *k1)
{
    if (!c || c->params->scheme != kSchemeBFV || c->params->plain_modulus < 2 || !k0 || !k1) return 0;
    bfv_reply_safe(c->params->N, c->params->plain_modulus, *k0, *k1);
    return bfv_reply_widths_ok(c->params->N, c->params->primes[0].q, *k0, *k1) ? 1 : 0;
}
// ---- reply compression (he355_kernels_bfv_reply.hip; the definition: bfv_reply_core.h, include/he355.h) -----------------------------
// [n][2][L][N] coefficient form -> n replies.  L > 1 is, by definition, bfv_mod_switch(L -> 1) followed by the L = 1 call: the L = 1
// ciphertexts pass through one pool block held for the call.
int he355_bfv_reply_compress(he355_ctx *c, int L, int k0, int k1, uint64_t n, const uint64_t *ct, void *bytes, uint64_t stride)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_reply_compress");
        plan_reply(*c->params, "he355_bfv_reply_compress", L, k0, k1, n, bytes, stride, ct, 2 * (u64)(L > 0 ? L : 0) * c->params->N);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (L > kBfvLevelMaxL) throw std::invalid_argument("he355_bfv_reply_compress: BFV modulus switching supports up to 16 data primes");
        if (!n) return;
        PoolBlock low;
        if (L > 1) {
            low = d.scoped_block((size_t)n * 2 * P.N * 8);
            launch_bfv_mod_switch(d.env(), d.bfv_drop_table_dev(), (int)P.Ltop, L, 1, n * 2, ct, low.get());
            ct = low.get();
        }
        launch_bfv_reply_pack(d.env(), k0, k1, n, ct, stride, bytes);
        HIPCHECK(hipGetLastError());
    });
}
// n replies -> plain [n][N] mod t, budget / noise_bits [n] int32 (either may be null).  Per chunk of at most 64 replies (as decrypt();
// never more than the batch chunk, he355_set_chunk): c1 unpacked, centred and lifted mod q_0 into client scratch, forward transform,
// product with the NTT-form secret key at prime 0 in place, inverse transform, then k_bfv_reply_finish adds c0's field, rounds, and
// gathers the largest residue's bit length in `budget` (or `noise_bits` when that is the only output), which k_bfv_noise_finish turns
// into the budget with 2^k1 in the place of q.  One transform less per reply than decrypt() spends: c0 is never transformed.
int he355_bfv_reply_decrypt(he355_ctx *c, int k0, int k1, uint64_t n, const void *bytes, uint64_t stride, uint64_t *plain, int32_t *budget, int32_t *noise_bits)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_reply_decrypt");
        plan_reply(*c->params, "he355_bfv_reply_decrypt", 1, k0, k1, n, bytes, stride, plain, c->params->N, true, budget, noise_bits);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!d.secret_key()) throw std::invalid_argument("he355_bfv_reply_decrypt: secret key not set (he355_set_secret_key)");
        if (!n) return;
        if (!bytes || !plain) throw std::invalid_argument("he355_bfv_reply_decrypt: null replies or null plaintext output");
        const size_t N = P.N;
        const u64 cmax = std::max<u64>(1, std::min<u64>(n, std::min<u64>(64, d.chunk_limit())));
        u64 *prod = d.client_scratch(cmax * N);
        int32_t *bits = budget ? budget : noise_bits;
        if (bits) HIPCHECK(hipMemsetAsync(bits, 0, n * sizeof(int32_t), d.stream()));
        for (u64 off = 0; off < n; off += cmax) {
            const u64 cnt = std::min<u64>(cmax, n - off);
            const unsigned char *src = static_cast<const unsigned char *>(bytes) + off * stride;
            launch_bfv_reply_lift(d.env(), k0, k1, cnt, src, stride, prod);
            launch_ntt_forward(d.env(), d.poly_view(prod, 1, N, 1), (u32)cnt);
            launch_bfv_noise_dot_sk(d.env(), 1, 2, cnt, prod, d.secret_key(), prod);
            launch_ntt_inverse(d.env(), d.poly_view(prod, 1, N, 1), (u32)cnt);
            launch_bfv_reply_finish(d.env(), k0, k1, P.plain_modulus, cnt, src, stride, prod, plain + off * N, bits ? bits + off : nullptr);
        }
        if (budget) launch_bfv_noise_finish(d.env(), n, budget, noise_bits, k1);
        HIPCHECK(hipGetLastError());
    });
}
int he355_bfv_seeded_encrypt(he355_ctx *c, int L, uint64_t n, const uint64_t *plain, uint64_t a_seed, uint64_t noise_seed, uint64_t first_index, uint64_t *c0)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_seeded_encrypt");
        plan_seeded_encrypt(*c->params, L, n, plain, a_seed, noise_seed, first_index, c0);
        DeviceContext &d = dev(c);
        d.use();
        seeded_c0(d, "he355_bfv_seeded_encrypt", L, n, plain, a_seed, noise_seed, first_index, c0);
        HIPCHECK(hipGetLastError());
    });
}
// polynomial 0 of he355_bfv_selector_encrypt with the seeded zero in the place of the public-key one: the same plants in the same places
int he355_bfv_seeded_selector_encrypt(he355_ctx *c, int L, int digit_bits, uint64_t n, uint64_t n_sel, uint64_t first_slot, uint64_t count, const uint64_t *sel,
                                      uint64_t a_seed, uint64_t noise_seed, uint64_t first_index, uint64_t *c0)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_seeded_selector_encrypt");
        const BfvSelectorPlan pl = plan_seeded_selector(*c->params, L, digit_bits, n, n_sel, first_slot, count, sel, a_seed, noise_seed, first_index, c0);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        seeded_c0(d, "he355_bfv_seeded_selector_encrypt", L, n, nullptr, a_seed, noise_seed, first_index, c0);
        launch_bfv_seeded_plant(d.env(), pl.tab, L, n, n_sel, first_slot, pl.depth, sel, P.plain_modulus, c0);
        HIPCHECK(hipGetLastError());
    });
}
// c0 [n][L][N] -> out [n][2][L][N]: c0 placed, the seeded half generated where it lies, then ONE transform in place over the half whose
// form has to change (ntt_form 0: c1 = iNTT(a); 1: c0 = NTT(c0)).  No scratch, so nothing to chunk; needs no key.
int he355_bfv_seeded_restore(he355_ctx *c, int L, int ntt_form, uint64_t n, const uint64_t *c0, uint64_t a_seed, uint64_t first_index, uint64_t *out)
{
    return guarded([&] {
        need_bfv(c, "he355_bfv_seeded_restore");
        plan_seeded_restore(*c->params, L, ntt_form, n, c0, first_index, out);
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        if (!n) return;
        const size_t N = P.N, LN = (size_t)L * N;
        launch_bfv_seeded_place(d.env(), L, n, c0, out);
        launch_bfv_seeded_gen(d.env(), L, n, a_seed, client::seeded_a_stream(first_index, 0), 64, out + LN, 2 * LN, nullptr);
        PolyView v = d.poly_view(out + (ntt_form ? 0 : LN), L, N, L);
        v.item_stride = 2 * LN;
        if (ntt_form) launch_ntt_forward(d.env(), v, (u32)n);
        else launch_ntt_inverse(d.env(), v, (u32)n);
        HIPCHECK(hipGetLastError());
    });
}
} // extern "C"
