// ckks_eval_mod.inc -- the fused combine-and-rescale step, the Chebyshev-basis polynomial evaluation on it and EvalMod: launch sequences and
// C ABI together.  Included by he355_api.hip alone, behind ckks_poly_raise.inc, whose table upload and plan walk (run_poly_plan) it shares.

// he355_combine_scalars_rescale: out [n][size][L - 1][N] = he355_rescale(he355_combine_scalars(...)) bit for bit, without the combined slab.
// The table (he355_combine_scalars' words) is uploaded once; per chunk -- the key-switch chunk, through for_each_chunk as rescale() takes it --
//   k_scalar_combine_row      row L - 1 of the combination alone -> `row` [nc size][N]
//   k_rows_inv_select         its inverse row pass -> S.rlr (raw rows of prime L - 1)
//   k_floor_colsn             the corrections under the L - 1 targets -> S.f, with the latency split of rescale_tail
//   k_floor_rows_combine      (sum_t a_t x_t + const - NTT(corrections)) * q_(L-1)^-1, the sums formed from the term rows themselves
// row: [min(chunk, n)][size][N] words the caller owns (the evaluation calls' pool block), or null: a pool block of this call's.
static void combine_scalars_rescale(DeviceContext &d, int L, int size, u64 n, const PolyTerm *terms, u64 n_terms, const u64 *h_scalars, const u64 *h_const, u64 *row,
                                    u64 *out)
{
    d.use();
    const size_t N = d.params().N, L1N = (size_t)(L - 1) * N;
    const size_t chunk = d.chunk_ops(n, L, false);
    const PoolBlock own = row ? PoolBlock() : d.scoped_block(std::min<u64>(chunk, n) * (size_t)size * N * 8);
    u64 *const rows = row ? row : own.get();
    const CombineTableDev t = upload_combine_table(d, L, terms, n_terms, h_scalars, h_const);
    ++d.counters().cheb.fused_steps;
    d.for_each_chunk(n, L, chunk, false, [&](u64 off, u64 nc, int which, const DeviceContext::Scratch &S, hipEvent_t) {
        const KernelEnv env = d.batch_env(which);
        launch_scalar_combine_row(env, L, size, nc, off, t.terms, n_terms, t.scalars, t.cst, rows);
        launch_rows_inv_select(env, L - 1, nc * (u64)size, rows, (u64)N, S.rlr);
        launch_floor_cols(env, L - 1, L - 1, nc * (u64)size, S.rlr, S.f, 0, 0, nullptr, 0, d.latency_shape(env, nc) ? kLatTargets : 1);
        launch_floor_rows_combine(env, L, size, nc, off, S.f, t.terms, n_terms, t.scalars, t.cst, out + off * (size_t)size * L1N);
    });
    HIPCHECK(hipGetLastError());
}

// the plan's public block, with the pool bytes at the context's batch chunk (he355_ckks_eval_poly_plan's rule)
static void cheb_plan_out(const PolyPlan &pl, u64 chunk, u64 n, he355_poly_plan_t *out)
{
    *out = pl.info;
    const u128 bytes = (u128)pl.words_per_ct * std::min<u64>(chunk, n) * 8, bound = bytes + ((u128)2 << 20);
    out->pool_bytes = !n ? 0 : bound > ~(u64)0 ? ~(u64)0 : (u64)bound;
}

extern "C" {
int he355_combine_scalars_rescale(he355_ctx *c, int L, int size, uint64_t n, const he355_term *terms, uint64_t n_terms, const uint64_t *scalars, const uint64_t *cst,
                                  uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_combine_scalars_rescale(*c->params, L, size, n, terms, n_terms, scalars, cst, out)) return; // nothing to combine: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        std::vector<PolyTerm> t((size_t)n_terms);
        for (size_t k = 0; k < t.size(); ++k) t[k] = {terms[k].d_ct, terms[k].L};
        combine_scalars_rescale(d, L, size, n, t.data(), n_terms, scalars, cst, nullptr, out);
    });
}
int he355_ckks_eval_chebyshev_plan(const he355_ctx *c, int L, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale, uint64_t n,
                                   he355_poly_plan_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (!out) throw std::invalid_argument("he355_ckks_eval_chebyshev_plan: null plan");
        const u64 chunk = c->dev ? c->dev->chunk_limit() : 1024;
        cheb_plan_out(plan_eval_chebyshev(*c->params, "he355_ckks_eval_chebyshev_plan", L, n, nullptr, coeffs, n_coeffs, log_baby, in_scale, out_scale, nullptr, false, chunk),
                      chunk, n, out);
    });
}
int he355_ckks_eval_chebyshev(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                              uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const PolyPlan pl = plan_eval_chebyshev(*c->params, "he355_ckks_eval_chebyshev", L, n, in, coeffs, n_coeffs, log_baby, in_scale, out_scale, out, true, 1024);
        if (pl.empty) return; // nothing to evaluate: no buffer is touched, no device asked for
        run_poly_plan(c, pl, "he355_ckks_eval_chebyshev", L, n, in, out, true);
    });
}
int he355_ckks_eval_mod_plan(const he355_ctx *c, int L, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale, int double_angles,
                             uint64_t n, he355_poly_plan_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (!out) throw std::invalid_argument("he355_ckks_eval_mod_plan: null plan");
        const u64 chunk = c->dev ? c->dev->chunk_limit() : 1024;
        cheb_plan_out(plan_eval_mod(*c->params, "he355_ckks_eval_mod_plan", L, n, nullptr, coeffs, n_coeffs, log_baby, in_scale, out_scale, double_angles, nullptr, false, chunk),
                      chunk, n, out);
    });
}
int he355_ckks_eval_mod(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const double *coeffs, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                        int double_angles, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const PolyPlan pl = plan_eval_mod(*c->params, "he355_ckks_eval_mod", L, n, in, coeffs, n_coeffs, log_baby, in_scale, out_scale, double_angles, out, true, 1024);
        if (pl.empty) return;
        run_poly_plan(c, pl, "he355_ckks_eval_mod", L, n, in, out, true);
    });
}
int he355_cheb_stats(he355_ctx *c, he355_cheb_stats_t *out, int reset)
{
    return guarded([&] {
        if (!out) throw std::invalid_argument("null pointer");
        *out = dev(c).cheb_stats(reset != 0);
    });
}
} // extern "C"
