// ckks_complex.inc -- complex CKKS slots: the complex codec, the complex scalar combination and complex coefficients in polynomial
// evaluation, C ABI and call sequences together.  Included by he355_api.hip alone, behind ckks_poly_raise.inc, whose combine_scalars and
// run_poly_plan it shares: a complex call differs from its real sibling in the residue pairs of its tables and in the kernel that reads them.

extern "C" {
int he355_ckks_encode_complex(he355_ctx *c, uint64_t n, const double *d_values, uint64_t count, double scale, uint64_t *d_plain)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_encode_complex(*c->params, n, d_values, count, scale, d_plain)) return;
        dev(c).ckks_encode(n, d_values, count, scale, d_plain, true);
    });
}
int he355_ckks_decode_complex(he355_ctx *c, int L, uint64_t n, const uint64_t *d_plain, double scale, double *d_out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        SlotRanges sr;
        if (plan_decode_complex(*c->params, "he355_ckks_decode_complex", L, n, d_plain, scale, nullptr, 0, false, d_out, sr)) return;
        dev(c).ckks_decode(L, n, d_plain, scale, d_out, nullptr, 0, true);
    });
}
int he355_ckks_decode_complex_slots(he355_ctx *c, int L, uint64_t n, const uint64_t *d_plain, double scale, const uint64_t *ranges, uint64_t n_ranges, double *d_out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        SlotRanges sr;
        if (plan_decode_complex(*c->params, "he355_ckks_decode_complex_slots", L, n, d_plain, scale, ranges, n_ranges, true, d_out, sr)) return;
        dev(c).ckks_decode(L, n, d_plain, scale, d_out, ranges, n_ranges, true);
    });
}
int he355_ckks_complex_unit(const he355_ctx *c, int L, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        cplx_units(*c->params, "he355_ckks_complex_unit", L, out);
    });
}
int he355_ckks_complex_scalar_residues(const he355_ctx *c, int L, double v_re, double v_im, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        cplx_scalar_residues(*c->params, "he355_ckks_complex_scalar_residues", L, v_re, v_im, out);
    });
}
int he355_combine_scalars_complex(he355_ctx *c, int L, int size, uint64_t n, const he355_term *terms, uint64_t n_terms, const uint64_t *scalars, const uint64_t *cst,
                                  uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (plan_combine_scalars(*c->params, L, size, n, terms, n_terms, scalars, cst, out, 2)) return; // nothing to combine: no buffer is touched, no device asked for
        DeviceContext &d = dev(c);
        std::vector<PolyTerm> t((size_t)n_terms);
        for (size_t k = 0; k < t.size(); ++k) t[k] = {terms[k].d_ct, terms[k].L};
        combine_scalars(d, L, size, n, t.data(), n_terms, scalars, cst, out, 2);
    });
}
int he355_ckks_eval_poly_complex_plan(const he355_ctx *c, int L, const double *re, const double *im, uint64_t n_coeffs, int log_baby, double in_scale, double out_scale,
                                      uint64_t n, he355_poly_plan_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        if (!out) throw std::invalid_argument("he355_ckks_eval_poly_complex_plan: null plan");
        const u64 chunk = c->dev ? c->dev->chunk_limit() : 1024;
        const PolyPlan pl = plan_eval_poly(*c->params, "he355_ckks_eval_poly_complex_plan", L, n, nullptr, re, n_coeffs, log_baby, in_scale, out_scale, nullptr, false,
                                           chunk, im, true);
        *out = pl.info;
        const u128 bytes = (u128)pl.words_per_ct * std::min<u64>(chunk, n) * 8, bound = bytes + ((u128)2 << 20); // (as he355_ckks_eval_poly_plan)
        out->pool_bytes = !n ? 0 : bound > ~(u64)0 ? ~(u64)0 : (u64)bound;
    });
}
int he355_ckks_eval_poly_complex(he355_ctx *c, int L, uint64_t n, const uint64_t *in, const double *re, const double *im, uint64_t n_coeffs, int log_baby,
                                 double in_scale, double out_scale, uint64_t *out)
{
    return guarded([&] {
        if (!c) throw std::invalid_argument("null context");
        const PolyPlan pl = plan_eval_poly(*c->params, "he355_ckks_eval_poly_complex", L, n, in, re, n_coeffs, log_baby, in_scale, out_scale, out, true, 1024, im, true);
        if (pl.empty) return; // nothing to evaluate: no buffer is touched, no device asked for
        run_poly_plan(c, pl, "he355_ckks_eval_poly_complex", L, n, in, out);
    });
}
} // extern "C"
