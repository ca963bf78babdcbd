// ckks_poly_raise.inc -- CKKS polynomial evaluation (the scalar combination under it) and the modulus raise: launch sequences and C ABI
// together.  Included by he355_api.hip alone.

// he355_combine_scalars: one launch of k_scalar_combine over `n` ciphertexts.  The table -- [n_terms] {slab, level} pairs, the scalars
// [n_terms][L], the constant [L] -- takes one region of the table ring (table_ring): calls may follow each other without a sync.
// halves = 2: he355_combine_scalars_complex -- scalars [n_terms][2][L], the constant [2][L], one launch of k_scalar_combine_cplx.
struct PolyTerm { const u64 *p; int L; };
// upload_combine_table: the table alone (the fused step of ckks_eval_mod.inc reads the same words).  count: he355_poly_stats takes the launch.
struct CombineTableDev { const u64 *terms, *scalars, *cst; };
static CombineTableDev upload_combine_table(DeviceContext &d, int L, const PolyTerm *terms, u64 n_terms, const u64 *h_scalars, const u64 *h_const, int halves = 1)
{
    const size_t Lh = (size_t)L * (size_t)halves;
    const size_t t_words = 2 * (size_t)n_terms, s_words = (size_t)n_terms * Lh, words = t_words + s_words + (h_const ? Lh : 0);
    std::vector<u64> h(words);
    for (size_t t = 0; t < n_terms; ++t) {
        h[2 * t] = (u64)(uintptr_t)terms[t].p;
        h[2 * t + 1] = (u64)terms[t].L; // (the kernel's row of the term: (c * size + k) * L_t + i)
    }
    std::memcpy(h.data() + t_words, h_scalars, s_words * 8);
    if (h_const) std::memcpy(h.data() + t_words + s_words, h_const, Lh * 8);
    const size_t bytes = (words * 8 + 255) & ~(size_t)255;
    u64 *d_tab = reinterpret_cast<u64 *>(d.table_ring(bytes));
    HIPCHECK(hipMemcpy(d_tab, h.data(), words * 8, hipMemcpyHostToDevice));
    return CombineTableDev{d_tab, d_tab + t_words, h_const ? d_tab + t_words + s_words : nullptr};
}
static void combine_scalars(DeviceContext &d, int L, int size, u64 n, const PolyTerm *terms, u64 n_terms, const u64 *h_scalars, const u64 *h_const, u64 *out, int halves = 1,
                            bool count = true)
{
    d.use();
    const CombineTableDev t = upload_combine_table(d, L, terms, n_terms, h_scalars, h_const, halves);
    if (halves == 2) {
        if (count) ++d.counters().poly.complex_combinations;
        launch_scalar_combine_cplx(d.batch_env(0, true), L, size, n, t.terms, n_terms, t.scalars, t.cst, out);
    } else {
        if (count) ++d.counters().poly.combinations;
        launch_scalar_combine(d.batch_env(0, true), L, size, n, t.terms, n_terms, t.scalars, t.cst, out);
    }
    HIPCHECK(hipGetLastError());
}
static void combine_scalars_rescale(DeviceContext &d, int L, int size, u64 n, const PolyTerm *terms, u64 n_terms, const u64 *h_scalars, const u64 *h_const, u64 *row,
                                    u64 *out); // (ckks_eval_mod.inc)

// The walk of a polynomial plan (poly_args.h), chunk by chunk in the key-switch chunk: he355_ckks_eval_poly and he355_ckks_eval_poly_complex.
// The power store and the temporaries are ONE pool block sized for the chunk, taken after the key check and before the first launch; every
// step is queued on the one stream.  cheb: a plan of he355_ckks_eval_chebyshev / he355_ckks_eval_mod -- its steps count in he355_cheb_stats and
// he355_poly_stats does not move; its fused steps (kPolyFused) share the row block at the plan's row_off.
static void run_poly_plan(he355_ctx *c, const PolyPlan &pl, const char *what, int L, u64 n, const u64 *in, u64 *out, bool cheb = false)
{
    DeviceContext &d = dev(c);
    d.use();
    const Params &P = d.params();
    d.require_keyswitch();
    if (!d.relin_key()) throw std::invalid_argument(std::string(what) + ": relinearization key not present"); // before anything is allocated
    const size_t chunk = d.chunk_ops(n, L, false);
    const PoolBlock blk = d.scoped_block((size_t)pl.words_per_ct * chunk * 8);
    const size_t N = P.N;
    Indexer pw{};
    pw.b1 = 1; pw.pairwise = 1;
    he355_poly_stats_t &ps = d.counters().poly;
    he355_cheb_stats_t &cs = d.counters().cheb;
    ++(cheb ? cs.calls : ps.calls);
    for (u64 off = 0; off < n; off += chunk) {
        const u64 nc = std::min<u64>(chunk, n - off);
        ++(cheb ? cs.chunks : ps.chunks);
        auto at = [&](int b) -> u64 * {
            const PolyBuf &B = pl.bufs[(size_t)b];
            if (B.kind == 0) return const_cast<u64 *>(in) + off * 2 * (size_t)B.L * N;
            if (B.kind == 1) return out + off * 2 * (size_t)B.L * N;
            return blk.get() + B.off * nc;
        };
        for (const PolyStep &s : pl.steps) {
            switch (s.op) {
            case kPolyMulRelin:
                ++(cheb ? cs.products : ps.products);
                if (s.angle) ++cs.double_angles;
                d.multiply_relin(s.L, nc, at(s.a), at(s.b), pw, s.rescale, at(s.dst));
                break;
            case kPolyDrop:
                ++(cheb ? cs.drops : ps.drops);
                d.mod_switch_drop(pl.bufs[(size_t)s.a].L, s.L, nc * 2, at(s.a), at(s.dst));
                break;
            case kPolyRescale:
                ++ps.rescales;
                d.rescale(s.L, 2, nc, at(s.a), at(s.dst));
                break;
            case kPolyAdd:
                ++(cheb ? cs.adds : ps.adds);
                d.addsub(s.L, 2, nc, at(s.a), at(s.b), pw, at(s.dst), false);
                break;
            case kPolyCombine: {
                std::vector<PolyTerm> t;
                for (int b : s.terms) t.push_back({at(b), pl.bufs[(size_t)b].L});
                if (cheb) ++cs.combinations;
                combine_scalars(d, s.L, 2, nc, t.data(), t.size(), s.scalars.data(), s.cst.empty() ? nullptr : s.cst.data(), at(s.dst), s.cplx ? 2 : 1, !cheb);
                break;
            }
            case kPolyFused: {
                std::vector<PolyTerm> t;
                for (int b : s.terms) t.push_back({at(b), pl.bufs[(size_t)b].L});
                combine_scalars_rescale(d, s.L, 2, nc, t.data(), t.size(), s.scalars.data(), s.cst.empty() ? nullptr : s.cst.data(), blk.get() + pl.row_off * nc, at(s.dst));
                break;
            }
            }
        }
    }
}

extern "C" {
int he355_combine_scalars(he355_ctx *c, int L, int size, uint64_t n, const he355_term *terms, uint64_t n_terms, const uint64_t *scalars, const uint64_t *cst, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_combine_scalars(*c->params, L, size, n, terms, n_terms, scalars, cst, out)) return; // nothing to combine: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        std::vector<PolyTerm> t((size_t)n_terms);
        for (size_t k = 0; k < t.size(); ++k) t[k] = {terms[k].d_ct, terms[k].L};
        combine_scalars(d, L, size, n, t.data(), n_terms, scalars, cst, out);
    });
}
int he355_ckks_scalar_residues(const he355_ctx *c, int L, double v, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        poly_scalar_residues(*c->params, "he355_ckks_scalar_residues", L, v, out);
    });
}
int he355_ckks_eval_poly_plan(const he355_ctx *c, int L, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale, uint64_t n,
                              he355_poly_plan_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (!out) throw std::invalid_argument("he355_ckks_eval_poly_plan: null plan");
        const u64 chunk = c->dev ? c->dev->chunk_limit() : 1024;
        const PolyPlan pl = plan_eval_poly(*c->params, "he355_ckks_eval_poly_plan", L, n, nullptr, coeffs, n_coeffs, log_baby, in_scale, out_scale, nullptr, false, chunk);
        *out = pl.info;
        // one block of min(chunk, n) times the plan's words, rounded up by a size class of the pool (at most 2 MiB: device_pool.h)
        const u128 bytes = (u128)pl.words_per_ct * std::min<u64>(chunk, n) * 8, bound = bytes + ((u128)2 << 20);
        out->pool_bytes = !n ? 0 : bound > ~(u64)0 ? ~(u64)0 : (u64)bound;
    });
}
// he355_ckks_eval_poly: the plan's steps (poly_args.h), walked by run_poly_plan
int he355_ckks_eval_poly(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                         uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const PolyPlan pl = plan_eval_poly(*c->params, "he355_ckks_eval_poly", L, n, in, coeffs, n_coeffs, log_baby, in_scale, out_scale, out, true, 1024);
        if (pl.empty) return; // nothing to evaluate: no buffer is touched, no device asked for
        run_poly_plan(c, pl, "he355_ckks_eval_poly", L, n, in, out);
    });
}
int he355_poly_stats(he355_ctx *c, he355_poly_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).poly_stats(reset != 0);
    });
}
// he355_ckks_mod_raise: row 0 of every polynomial copied on the stream, then chunk by chunk (the key-switch chunk, in ciphertexts) the
// inverse row pass of row 0 into a compact tail [nc size][N] from the pool (k_rows_inv_select, prime 0), the fused column kernel
// (k_raise_cols; N = 1024 has no column pass: k_raise_lift on the finished coefficients) and the forward row pass over rows 1 .. L_to - 1
// in place.  A chunk of fewer than CUs / 4 polynomials deals the targets of a column to raise_tsplit blocks, as the latency shape of the
// key switch does -- unless the latency shapes are switched off (he355_set_latency_max(0)).
int he355_ckks_mod_raise(he355_ctx *c, int L_in, int L_to, int size, uint64_t n, const uint64_t *in, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_mod_raise(*c->params, L_in, L_to, size, n, in, out)) return; // nothing to raise: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        d.use();
        const Params &P = d.params();
        const size_t N = P.N;
        ++d.counters().raise.calls;
        const u64 chunk = std::min<u64>(d.chunk_limit(), n);
        const PoolBlock tail = L_to > 1 ? d.scoped_block((size_t)chunk * size * N * 8) : PoolBlock();
        const bool split_on = d.limits().lat_auto || d.limits().lat_max > 0;
        for (u64 off = 0; off < n; off += chunk) {
            const u64 np = std::min<u64>(chunk, n - off) * (u64)size;
            const u64 *src = in + off * size * (size_t)L_in * N;
            u64 *dst = out + off * size * (size_t)L_to * N;
            ++d.counters().raise.chunks;
            HIPCHECK(hipMemcpy2DAsync(dst, (size_t)L_to * N * 8, src, (size_t)L_in * N * 8, N * 8, (size_t)np, hipMemcpyDeviceToDevice, d.stream()));
            if (L_to > 1) {
                launch_rows_inv_select(d.env(), 0, np, src, (u64)L_in * N, tail.get());
                if (P.logn1 == 0) {
                    ++d.counters().raise.streaming_launches;
                    launch_raise_lift(d.env(), L_to, 1, np, tail.get(), dst);
                } else {
                    const int tsplit = split_on ? raise_tsplit(np, L_to, d.compute_units()) : 1;
                    ++d.counters().raise.fused_launches;
                    if (tsplit > 1) ++d.counters().raise.split_launches;
                    launch_raise_cols(d.env(), L_to, np, tail.get(), dst, tsplit);
                }
                PolyView pv = d.poly_view(dst + N, L_to - 1, N, L_to);
                pv.item_stride = (u64)L_to * N;
                for (int j = 1; j < L_to; ++j) pv.prime_of[j - 1] = (unsigned char)j;
                launch_rows_fwd(d.env(), pv, (u32)np);
            }
        }
        HIPCHECK(hipGetLastError());
    });
}
// he355_ckks_lift_centred: one streaming launch
int he355_ckks_lift_centred(he355_ctx *c, int L_to, uint64_t n_polys, const uint64_t *coeff, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_lift_centred(*c->params, L_to, n_polys, coeff, out)) return;
        DeviceContext &d = dev(c);
        d.use();
        ++d.counters().raise.streaming_launches;
        launch_raise_lift(d.env(), L_to, 0, n_polys, coeff, out);
        HIPCHECK(hipGetLastError());
    });
}
int he355_raise_stats(he355_ctx *c, he355_raise_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).raise_stats(reset != 0);
    });
}
} // extern "C"
