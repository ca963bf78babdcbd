// hoisted_rotations.inc -- the hoisted rotations, the baby-step/giant-step linear transform and he355_plain_extend_special: launch
// sequences and C ABI together.  Included by he355_api.hip alone.  The permuted keys and the tables are the key store's (DeviceContext).

// What a hoisted call sets up before its first launch.  Every keyed element's Galois key must be installed: refused before anything is
// built.  Then per element its table -- the NTT-domain permutation, or (coeff) the coefficient-form gather -- and its permuted key
// (hoist_key; null: the identity, which gets a table only with ident_tables: the blocks of rotate_hoisted are finished through one),
// and the identity's permutation for the digit lift of the NTT-domain pipeline.
struct HoistSetup {
    std::vector<const uint32_t *> table;
    std::vector<const u64 *> key;
    const uint32_t *ident = nullptr;
};
// (what: the call's name in front of the refusal; null: the bare message of the first hoisted calls)
static void hoist_require_keys(DeviceContext &d, const std::vector<uint32_t> &elts, const char *what = nullptr)
{
    for (uint32_t e : elts)
        if (e != 1 && !d.galois_key(e)) throw std::invalid_argument(what ? std::string(what) + ": Galois key not present" : std::string("Galois key not present"));
}
static HoistSetup hoist_setup(DeviceContext &d, const std::vector<uint32_t> &elts, bool coeff, bool ident_tables, const char *what = nullptr)
{
    hoist_require_keys(d, elts, what);
    const size_t n_elts = elts.size();
    HoistSetup hs{std::vector<const uint32_t *>(n_elts, nullptr), std::vector<const u64 *>(n_elts, nullptr), nullptr};
    bool keyed = false;
    for (size_t r = 0; r < n_elts; ++r) {
        const uint32_t e = elts[r];
        if (e != 1 || ident_tables) hs.table[r] = coeff ? d.gather(e) : d.perm(e);
        if (e != 1) hs.key[r] = d.hoist_key(e);
        keyed |= e != 1;
    }
    if (keyed && !coeff) hs.ident = d.perm(1);
    return hs;
}
// The one digit lift of a chunk of a hoisted call, counted in he355_hoist_stats: the input's c1 as it lies (the identity's permutation)
// through k_k1's inverse row pass -- c2n, c2r; nothing of c01 is written -- and k_k2n; coeff: (c0, 0) into B.e for the BFV tail, and
// k_k2n on the coefficients of c1.  op 0 of the chunk is ciphertext `off` of `in`.
static void hoist_digit_lift(DeviceContext &d, const KernelEnv &env, int L, u64 nc, u64 off, const u64 *in, const KsBuffers &B, bool coeff, const uint32_t *ident)
{
    const Params &P = d.params();
    const size_t LN = (size_t)L * P.N;
    ++d.counters().hoist.digit_lifts;
    if (coeff) {
        const u64 *a = in + off * 2 * LN;
        launch_hoist_addend_coeff(env, L, nc, a, B.e);
        launch_k2(env, L, nc, B, a + LN, 2 * LN);
        return;
    }
    K1Operands k1;
    k1.mode = K1_GALOIS; k1.a = in; k1.op_offset = off; k1.perm = ident;
    k1.no_c1 = k1.no_c0n = true;
    launch_k1(env, L, nc, k1, B);
    launch_k2(env, L, nc, B);
}

extern "C" {
// Hoisted rotations: out block r = sigma_g(c0 + u0, u1) of every input under element pl.elts[r], (u0, u1) the key switch of the input's
// c1 itself under hoist_key(g) -- the digit lift (the inverse row pass and k_k2n, or k_k2n on the coefficients) runs ONCE per chunk and
// the slab S.ks.d is then read by every element's key product.  One stream only: the slab and the sums' scratch are reused from element
// to element, and the plain sum read-modify-writes `out` in launch order.  Per element the unfused tail (k_k3 on all primes, the floor
// step's column and row halves with no addend; BFV coefficient form: the two BFV tail kernels onto (c0, 0)) into scratch, then the
// finishing kernel.  plain (optional, NTT pipeline only): [n_elts][L][N], out [n][2][L][N] = sum_r plain[r] (.) block r.
// Counted in he355_hoist_stats, in no field of he355_path_stats.
static int hoisted_call(he355_ctx *c, const char *what, int L, int ntt_form, uint64_t n, const uint64_t *in, const uint32_t *elts, const int32_t *steps, uint64_t n_elts,
                        const uint64_t *plain, uint64_t *out, bool plain_sum)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const HoistPlan pl = plan_rotate_hoisted(*c->params, what, L, ntt_form, n, in, elts, steps, n_elts, plain, out, plain_sum);
        if (pl.empty) return; // nothing to rotate: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const bool coeff = P.scheme == kSchemeBFV && !ntt_form;
        const HoistSetup hs = hoist_setup(d, pl.elts, coeff, true);
        const size_t N = P.N, LN = (size_t)L * N;
        const int SP = (int)P.K - 1;
        d.for_each_chunk(n, L, d.chunk_ops(n, L, false), false, [&](u64 off, u64 nc, int, DeviceContext::Scratch S, hipEvent_t) {
            const KernelEnv env = d.batch_env(0, !coeff);
            const KsBuffers &B = S.ks; // (c01: the arena's [nc][2][L][N], every element's sums before the permutation)
            const u64 *a = in + off * 2 * LN;
            if (pl.keyed) hoist_digit_lift(d, env, L, nc, off, in, B, coeff, hs.ident);
            for (size_t r = 0; r < pl.elts.size(); ++r) {
                u64 *o = plain ? out + off * 2 * LN : out + ((u64)r * n + off) * 2 * LN;
                const u64 *pt = plain ? plain + r * LN : nullptr;
                if (!hs.key[r]) { // the identity
                    if (pt) launch_hoist_finish_ntt(env, L, nc, nullptr, a, hs.table[r], o, pt, r == 0);
                    else HIPCHECK(hipMemcpyAsync(o, a, nc * 2 * LN * 8, hipMemcpyDeviceToDevice, env.stream));
                    continue;
                }
                ++d.counters().hoist.key_products;
                ++d.counters().hoist.mod_downs; // (every element pays its own)
                launch_k3(env, L, nc, B, hs.key[r]);
                if (coeff) {
                    launch_bfv_tail_sp(env, nc * 2, B.tpr, S.rlr);
                    launch_bfv_tail_fin(env, L, nc, B.t, S.rlr, B.c01, B.c01_item_stride, B.e, 2 * LN);
                    launch_hoist_finish_coeff(env, L, nc, B.c01, hs.table[r], o);
                } else {
                    d.floor_step(env, SP, L, 2, nc, B.tpr, B.e, {B.t, 2 * LN, LN}, {}, {B.c01, B.c01_item_stride, LN});
                    launch_hoist_finish_ntt(env, L, nc, B.c01, a, hs.table[r], o, pt, r == 0);
                }
            }
        });
        HIPCHECK(hipGetLastError());
    });
}
int he355_apply_galois_hoisted(he355_ctx *c, int L, int ntt_form, uint64_t n, const uint64_t *in, const uint32_t *elts, uint64_t n_elts, uint64_t *out)
{
    if (n_elts && !elts) { g_last_error = "he355_apply_galois_hoisted: null elements"; return HE355_E_INVALID_ARGS; }
    return hoisted_call(c, "he355_apply_galois_hoisted", L, ntt_form, n, in, elts, nullptr, n_elts, nullptr, out, false);
}
int he355_rotate_hoisted(he355_ctx *c, int L, int ntt_form, uint64_t n, const uint64_t *in, const int32_t *steps, uint64_t n_steps, uint64_t *out)
{
    return hoisted_call(c, "he355_rotate_hoisted", L, ntt_form, n, in, nullptr, steps, n_steps, nullptr, out, false);
}
int he355_rotate_hoisted_plain_sum(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const int32_t *steps, uint64_t n_steps, const uint64_t *plain, uint64_t *out)
{
    return hoisted_call(c, "he355_rotate_hoisted_plain_sum", L, 1, n, in, nullptr, steps, n_steps, plain, out, true);
}
// The lazy-mod-down plain sum: out [n][2][L][N] = B + moddown(A), A = sum_r plain_qp[r] (.) sigma_r(key product r) accumulated in the
// extended basis Q P, B = the part that needs no key accumulated in Q (the definition: include/he355.h).  The lift runs as in
// rotate_hoisted; every keyed element then pays launch_k3 and ONE accumulate launch, and the mod-down runs once per chunk.  No scratch
// of its own: B.c01 holds the Q part of A, B.tp its P part (k_k3 leaves the special prime's sums in B.tpr, after its inverse row pass;
// the accumulate kernel's special-prime waves transform them back -- k3_body.inc is untouched), the output chunk itself holds B and
// B.e the corrections.  One stream; NTT-domain pipeline only.
int he355_rotate_hoisted_plain_sum_lazy(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const int32_t *steps, uint64_t n_steps, const uint64_t *plain_qp,
                                        uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const HoistPlan pl = plan_rotate_hoisted(*c->params, "he355_rotate_hoisted_plain_sum_lazy", L, 1, n, in, nullptr, steps, n_steps, plain_qp, out, true, true);
        if (pl.empty) return; // nothing to sum: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const HoistSetup hs = hoist_setup(d, pl.elts, false, false);
        const size_t N = P.N, LN = (size_t)L * N;
        const int SP = (int)P.K - 1;
        d.for_each_chunk(n, L, d.chunk_ops(n, L, false), false, [&](u64 off, u64 nc, int, DeviceContext::Scratch S, hipEvent_t) {
            const KernelEnv env = d.batch_env(0, true);
            const KsBuffers &B = S.ks;
            const u64 *a = in + off * 2 * LN;
            u64 *o = out + off * 2 * LN;
            if (pl.keyed) hoist_digit_lift(d, env, L, nc, off, in, B, false, hs.ident);
            bool first_a = true, first_b = true;
            for (size_t r = 0; r < pl.elts.size(); ++r) {
                const u64 *pt = plain_qp + r * (LN + N);
                if (!hs.key[r]) {
                    launch_hoist_acc_qp(env, L, nc, nullptr, nullptr, a, nullptr, pt, nullptr, 0, nullptr, o, false, first_b);
                } else {
                    ++d.counters().hoist.key_products;
                    launch_k3(env, L, nc, B, hs.key[r]);
                    launch_hoist_acc_qp(env, L, nc, B.t, B.tpr, a, hs.table[r], pt, B.c01, B.c01_item_stride, B.tp, o, first_a, first_b);
                    first_a = false;
                }
                first_b = false;
            }
            if (!pl.keyed) return;
            ++d.counters().hoist.mod_downs; // one per chunk, however many elements
            PolyView pv = d.poly_view(B.tp, 1, N, 1);
            pv.prime_of[0] = (unsigned char)SP;
            launch_rows_inv(env, pv, (u32)(nc * 2));
            d.floor_step(env, SP, L, 2, nc, B.tp, B.e, {B.c01, B.c01_item_stride, LN}, {o, 2 * LN, LN}, {o, 2 * LN, LN});
        });
        HIPCHECK(hipGetLastError());
    });
}
// The baby-step/giant-step linear transform on the hoisted rotations (the definition: include/he355.h).  Per chunk: ONE digit lift of the
// input, per used keyed baby launch_k3 and the rotate kernel into the baby store (T_i = sigma(S_i) with P sigma(c0) folded in; the
// identity: (P c0, P c1), streaming); then per used giant row the inner sum over its used terms -- straight into the accumulator for the
// identity row; for a keyed row into a Q P block, its mod-down into S.ks.c01 (free: k_k3 unfused never writes it), that ciphertext's own
// digit lift and key product, and the rotate kernel's accumulate form -- and the last mod-down into `out`.  The key-switch scratch is
// the chunk's arena, reused from step to step: one stream only.  The store and the two blocks come from the pool before the first launch;
// the term table lies in the context's table ring (table_ring).
int he355_linear_transform_bsgs(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const int32_t *baby, uint64_t n_baby, const int32_t *giant, uint64_t n_giant,
                                const uint64_t *plain_qp, const uint8_t *mask, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const BsgsPlan pl = plan_linear_transform_bsgs(*c->params, L, n, in, baby, n_baby, giant, n_giant, plain_qp, mask, out);
        if (pl.empty) return; // nothing to transform: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t N = P.N, LN = (size_t)L * N, QP = LN + N;
        const int SP = (int)P.K - 1;
        auto used_row = [&](size_t j) { return pl.row_first[j + 1] > pl.row_first[j]; };
        // the elements of the used steps, babies then giant rows (a step no kept term names counts as the identity: no key, no table)
        std::vector<uint32_t> elts(n_baby + n_giant, 1);
        for (size_t i = 0; i < n_baby; ++i)
            if (pl.slot[i] >= 0) elts[i] = pl.baby[i];
        for (size_t j = 0; j < n_giant; ++j)
            if (used_row(j)) elts[n_baby + j] = pl.giant[j];
        hoist_require_keys(d, elts, "he355_linear_transform_bsgs"); // before anything is allocated
        // the chunk: the key-switch chunk (chunk_ops: the batch chunk, halved until the arena is reserved); the pool blocks are sized for it
        const size_t chunk = d.chunk_ops(n, L, false);
        const PoolBlock store = d.scoped_block(bsgs_store_bytes((size_t)pl.slots, chunk, L, N));
        const PoolBlock blk_e = pl.keyed_rows ? d.scoped_block(bsgs_block_bytes(chunk, L, N)) : PoolBlock();
        const PoolBlock blk_a = d.scoped_block(bsgs_block_bytes(chunk, L, N));
        const HoistSetup hs = hoist_setup(d, elts, false, false, "he355_linear_transform_bsgs"); // (the permuted keys: the first launches)
        const uint32_t *const *bperm = hs.table.data(), *const *gperm = hs.table.data() + n_baby;
        const u64 *const *bkey = hs.key.data(), *const *gkey = hs.key.data() + n_baby;
        const uint32_t *ident = d.perm(1);
        // the term table goes through the table ring: a pool block written by a host copy would be outside the stream order that makes a
        // pool release safe (device_pool.h), and a second call could rewrite it under this call's queued launches
        const size_t t_bytes = (pl.terms.size() * 4 + 255) & ~(size_t)255;
        const uint32_t *const d_terms = reinterpret_cast<const uint32_t *>(d.table_ring(t_bytes));
        HIPCHECK(hipMemcpy(const_cast<uint32_t *>(d_terms), pl.terms.data(), pl.terms.size() * 4, hipMemcpyHostToDevice));
        u64 *const st = store.get();
        d.for_each_chunk(n, L, chunk, false, [&](u64 off, u64 nc, int, DeviceContext::Scratch S, hipEvent_t) {
            const KernelEnv env = d.batch_env(0, true);
            const KsBuffers &B = S.ks;
            const u64 *a = in + off * 2 * LN;
            u64 *o = out + off * 2 * LN;
            u64 *eq = blk_e.get(), *ep = eq ? eq + nc * 2 * LN : nullptr; // [nc][2][L][N], then [nc][2][N]
            u64 *aq = blk_a.get(), *ap = aq + nc * 2 * LN;
            const u64 slot_words = nc * 2 * QP;
            auto rows_inv_p = [&](u64 *p) {
                PolyView pv = d.poly_view(p, 1, N, 1);
                pv.prime_of[0] = (unsigned char)SP;
                launch_rows_inv(env, pv, (u32)(nc * 2));
            };
            if (pl.keyed_babies) hoist_digit_lift(d, env, L, nc, off, in, B, false, ident);
            for (size_t i = 0; i < n_baby; ++i) {
                if (pl.slot[i] < 0) continue;
                u64 *t = st + (u64)pl.slot[i] * slot_words; // [nc][2][L + 1][N]
                if (!bkey[i]) {
                    launch_bsgs_ident(env, L, nc, a, t);
                    continue;
                }
                ++d.counters().hoist.key_products;
                launch_k3(env, L, nc, B, bkey[i]);
                launch_hoist_rot_qp(env, L, nc, B.t, B.tpr, a, bperm[i], t, QP, t + LN, QP, false);
            }
            bool first = true; // the accumulator starts with the first used row
            for (size_t j = 0; j < n_giant; ++j) {
                if (!used_row(j)) continue;
                const uint32_t *terms = d_terms + 2 * pl.row_first[j];
                const u64 n_terms = pl.row_first[j + 1] - pl.row_first[j];
                const u64 *prow = plain_qp + (u64)j * n_baby * QP;
                ++d.counters().hoist.inner_sums;
                if (!gkey[j]) {
                    launch_bsgs_inner(env, L, nc, st, prow, terms, n_terms, aq, ap, !first);
                } else {
                    launch_bsgs_inner(env, L, nc, st, prow, terms, n_terms, eq, ep, false);
                    ++d.counters().hoist.mod_downs;
                    rows_inv_p(ep);
                    d.floor_step(env, SP, L, 2, nc, ep, B.e, {eq, 2 * LN, LN}, {}, {B.c01, B.c01_item_stride, LN});
                    hoist_digit_lift(d, env, L, nc, 0, B.c01, B, false, ident);
                    ++d.counters().hoist.key_products;
                    launch_k3(env, L, nc, B, gkey[j]);
                    launch_hoist_rot_qp(env, L, nc, B.t, B.tpr, B.c01, gperm[j], aq, LN, ap, N, !first);
                }
                first = false;
            }
            ++d.counters().hoist.mod_downs;
            rows_inv_p(ap);
            d.floor_step(env, SP, L, 2, nc, ap, B.e, {aq, 2 * LN, LN}, {}, {o, 2 * LN, LN});
        });
        HIPCHECK(hipGetLastError());
    });
}
uint64_t he355_linear_transform_bsgs_scratch_bytes(const he355_ctx *c, int L, uint64_t n, uint64_t n_baby)
{
    if (!c || L < 1 || (size_t)L > c->params->Ltop) return 0;
    return bsgs_scratch_bytes(c->dev ? c->dev->chunk_limit() : 1024, *c->params, L, n, n_baby);
}
// plain_ntt [n][L][N] NTT form -> plain_qp [n][L + 1][N]: the rows copied and row L = NTT_P of the coefficients of row 0, centred
// (he355_plain_extend_special).  mismatch (optional, one device word): the (coefficient, prime >= 1) pairs that disagree with row 0.
int he355_plain_extend_special(he355_ctx *c, int L, uint64_t n, const uint64_t *plain_ntt, uint64_t *plain_qp, uint64_t *mismatch)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_plain_extend(*c->params, L, n, plain_ntt, plain_qp)) return;
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t N = P.N;
        const int Lc = mismatch ? L : 1, SP = (int)P.K - 1;
        if (mismatch) HIPCHECK(hipMemsetAsync(mismatch, 0, 8, d.stream()));
        const u64 chunk = std::max<u64>(1, std::min<u64>(n, ((u64)1 << 27) / ((u64)Lc * N * 8)));
        const PoolBlock tmp = d.scoped_block((size_t)chunk * Lc * N * 8);
        for (u64 off = 0; off < n; off += chunk) {
            const u64 cnt = std::min<u64>(chunk, n - off);
            const u64 *src = plain_ntt + off * L * N;
            u64 *dst = plain_qp + off * (L + 1) * N;
            HIPCHECK(hipMemcpy2DAsync(tmp.get(), (size_t)Lc * N * 8, src, (size_t)L * N * 8, (size_t)Lc * N * 8, (size_t)cnt, hipMemcpyDeviceToDevice, d.stream()));
            launch_ntt_inverse(d.env(), d.poly_view(tmp.get(), Lc, N, Lc), (u32)cnt);
            launch_plain_extend(d.env(), L, cnt, src, tmp.get(), Lc, dst, mismatch);
            PolyView pv = d.poly_view(dst + (size_t)L * N, 1, N, 1);
            pv.item_stride = (u64)(L + 1) * N;
            pv.prime_of[0] = (unsigned char)SP;
            launch_ntt_forward(d.env(), pv, (u32)cnt);
        }
        HIPCHECK(hipGetLastError());
    });
}
} // extern "C"
