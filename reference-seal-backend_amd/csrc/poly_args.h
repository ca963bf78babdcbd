// poly_args.h -- the argument checks of he355_combine_scalars and he355_ckks_scalar_residues and the host plan of he355_ckks_eval_poly
// (power tree, split tree, levels, scales, integer scalars, buffers), made ONCE per call in the style of hoist_args.h: the C ABI function
// (ckks_poly_raise.inc) runs them before it asks for a device -- a refusal is HE355_E_INVALID_ARGS whether a device exists or not -- and
// then only walks the plan's steps.  Whether the relinearization key is installed is the device context's to know.
// Host-only on purpose: no HIP header, so tests/ckks_eval_poly_args_main.cpp runs every check at its edges under the sanitizers.
// The definition the plan implements is written out in include/he355.h; tests/ckks_eval_poly_ref.py restates it on the oracle.
// he355_combine_scalars_complex and he355_ckks_eval_poly_complex (ckks_complex.inc) take the same checks and the same planner under their
// own names: two residues per scalar (halves = 2), a coefficient a (re, im) pair (cplx) -- tests/ckks_complex_args_main.cpp.
#pragma once
#include <cmath>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/he355.h"
#include "bfv_pir_args.h"
#include "cplx_args.h"
#include "poly_core.h"

namespace he355 {

// ---- he355_ckks_scalar_residues ----------------------------------------------------------------------------------------------------
inline void poly_scalar_residues(const Params &p, const std::string &w, int L, double v, u64 *out)
{
    check_level(p, w, L);
    if (!out) throw std::invalid_argument(w + ": null output");
    u128 mag;
    bool neg;
    if (!poly_scalar_integer(v, mag, neg)) throw std::invalid_argument(w + ": the scalar is not finite or not below 2^126 in magnitude");
    for (int i = 0; i < L; ++i) out[i] = poly_scalar_residue(mag, neg, p.primes[i].q);
}

// ---- he355_combine_scalars -----------------------------------------------------------------------------------------------------------
// True: n == 0, or no term and no constant -- the call touches nothing.  halves = 2: he355_combine_scalars_complex under its own name --
// scalars [n_terms][2][L], cst [2][L], every other rule the same.
// out_rows: the rows of a polynomial of `out` (he355_combine_scalars_rescale, cheb_args.h, writes L - 1 of them under its own name `w`).
inline bool plan_combine_scalars(const Params &p, const std::string &w, int L, int size, u64 n, const he355_term *terms, u64 n_terms, const u64 *scalars, const u64 *cst,
                                 const u64 *out, int halves, int out_rows)
{
    check_level(p, w, L);
    if (size < 2 || size > 3) throw std::invalid_argument(w + ": ciphertext size must be 2 or 3");
    if (n_terms > ((u64)1 << 20)) throw std::invalid_argument(w + ": too many terms for one call (at most 2^20)");
    if (n_terms && (!terms || !scalars)) throw std::invalid_argument(w + ": null terms or scalars");
    for (u64 t = 0; t < n_terms; ++t) {
        if (terms[t].L < L || (size_t)terms[t].L > p.Ltop) throw std::invalid_argument(w + ": term " + std::to_string(t) + " lies at a level below the call's or above the top");
        for (int i = 0; i < halves * L; ++i)
            if (scalars[t * (u64)(halves * L) + (u64)i] >= p.primes[i % L].q) throw std::invalid_argument(w + ": a scalar of term " + std::to_string(t) + " is not a canonical residue");
    }
    if (cst)
        for (int i = 0; i < halves * L; ++i)
            if (cst[i] >= p.primes[i % L].q) throw std::invalid_argument(w + ": the constant is not a canonical residue");
    // every slab in words, formed in 128 bits: 2^60 words (2^63 bytes) is the most one may span
    const u128 cap = (u128)1 << 60, out_w = (u128)n * (u128)size * (u128)out_rows * p.N;
    if (n > cap || out_w > cap || (u128)n * (u128)size * (u128)L * p.N > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    for (u64 t = 0; t < n_terms; ++t)
        if ((u128)n * (u128)size * (u128)terms[t].L * p.N > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    if (n == 0 || (n_terms == 0 && !cst)) return true;
    if (n_terms == 0) throw std::invalid_argument(w + ": a constant alone is no ciphertext (no term)");
    if (!out) throw std::invalid_argument(w + ": null output");
    const AddrRange ro = word_range(w, out, (u64)out_w);
    for (u64 t = 0; t < n_terms; ++t) {
        if (!terms[t].d_ct) throw std::invalid_argument(w + ": term " + std::to_string(t) + " is null");
        if (ro.overlaps(word_range(w, terms[t].d_ct, (u64)((u128)n * (u128)size * (u128)terms[t].L * p.N))))
            throw std::invalid_argument(w + ": `d_out` overlaps term " + std::to_string(t));
    }
    return false;
}
inline bool plan_combine_scalars(const Params &p, int L, int size, u64 n, const he355_term *terms, u64 n_terms, const u64 *scalars, const u64 *cst, const u64 *out,
                                 int halves = 1)
{
    return plan_combine_scalars(p, halves == 2 ? "he355_combine_scalars_complex" : "he355_combine_scalars", L, size, n, terms, n_terms, scalars, cst, out, halves, L);
}

// ---- he355_ckks_eval_poly --------------------------------------------------------------------------------------------------------------
// A buffer of the call: [nc][2][L][N] per chunk of nc ciphertexts.  kind 0: d_in, 1: d_out, 2: the pool block at word `off` * nc.
struct PolyBuf { int kind; u64 off; int L; };
enum PolyOp { kPolyMulRelin, kPolyDrop, kPolyCombine, kPolyRescale, kPolyAdd, kPolyFused }; // kPolyFused: he355_combine_scalars_rescale at L, dst at L - 1
enum PolyBasis { kBasisMonomial = 0, kBasisChebyshev = 1 };
struct PolyStep {
    PolyStep(PolyOp o, int l) : op(o), L(l) {}
    PolyOp op;
    int L;                     // the level the op runs at (its operands'; a drop: the target level, `a` at its buffer's own)
    int a = -1, b = -1, dst = -1; // buffers
    std::vector<int> terms;    // kPolyCombine: the term buffers ...
    std::vector<u64> scalars;  // ... [terms][L] residues ...
    std::vector<u64> cst;      // ... and the constant [L], empty: none
    bool cplx = false;         // he355_ckks_eval_poly_complex: scalars [terms][2][L], cst [2][L] (k_scalar_combine_cplx)
    bool rescale = true;       // kPolyMulRelin: with the rescale (a Chebyshev power's product goes without: dst at L)
    bool angle = false;        // kPolyMulRelin: the square of a double-angle step of he355_ckks_eval_mod
};
struct PolyPlan {
    he355_poly_plan_t info{};
    std::vector<PolyBuf> bufs;
    std::vector<PolyStep> steps;
    u64 words_per_ct = 0; // pool words per ciphertext of a chunk
    u64 row_off = 0;      // the Chebyshev basis: word `row_off` * nc of the pool block starts the fused steps' row block [nc][2][N]
    bool empty = false;   // n == 0
};

inline int poly_clog2(u64 k) // ceil(log2 k), k >= 1
{
    int r = 0;
    while (((u64)1 << r) < k) ++r;
    return r;
}

class PolyPlanner {
public:
    PolyPlanner(const Params &p, const std::string &w, int L, int log_baby, double in_scale, bool cplx = false, int basis = kBasisMonomial)
        : P(p), w_(w), L_(L), m_((u64)1 << log_baby), cplx_(cplx), cheb_(basis == kBasisChebyshev)
    {
        level_[1] = L;
        scale_[1] = in_scale;
    }
    // A coefficient: the real call's has im = 0.  Zero when both parts are.
    struct Coef {
        double re, im;
        bool zero() const { return re == 0.0 && im == 0.0; }
    };
    typedef std::vector<Coef> Poly; // trimmed: the last coefficient is not zero (or the vector is empty)
    static Poly trimmed(const Coef *c, u64 n)
    {
        while (n && c[n - 1].zero()) --n;
        return Poly(c, c + n);
    }
    static Poly trimmed(const double *re, const double *im, u64 n)
    {
        Poly p((size_t)n);
        for (u64 k = 0; k < n; ++k) p[(size_t)k] = {re[k], im ? im[k] : 0.0};
        return trimmed(p.data(), n);
    }
    u64 giant_below(u64 deg) const // the largest m 2^j <= deg (deg >= m)
    {
        u64 e = m_;
        while (2 * e <= deg) e *= 2;
        return e;
    }
    // p = lo + (the basis element of e) * hi at e = the largest giant <= deg p; lo trimmed.  Monomials: the two halves of the list.  The
    // Chebyshev basis (T_k = 2 T_e T_(k-e) - T_(2e-k) for k > e; 2e > deg): hi[0] = c_e, and for k = e + 1 .. deg in increasing order
    // hi[k - e] = 2.0 * c_k, lo[2e - k] = lo[2e - k] - c_k.  A coefficient that becomes non-finite here is refused.
    void split(const Poly &p, u64 e, Poly &hi, Poly &lo) const
    {
        if (!cheb_) {
            hi.assign(p.begin() + e, p.end());
            lo = trimmed(p.data(), e);
            return;
        }
        hi.assign(p.size() - e, Coef{0.0, 0.0});
        lo.assign(p.begin(), p.begin() + e);
        hi[0] = p[e];
        for (u64 k = e + 1; k < p.size(); ++k) {
            hi[k - e] = {2.0 * p[k].re, 0.0};
            lo[2 * e - k].re = lo[2 * e - k].re - p[k].re;
            if (!std::isfinite(hi[k - e].re) || !std::isfinite(lo[2 * e - k].re)) throw std::invalid_argument(w_ + ": a coefficient becomes non-finite in the Chebyshev split");
        }
        lo = trimmed(lo.data(), e);
    }
    int depth(const Poly &p) const // deg p >= 1
    {
        const u64 deg = p.size() - 1;
        if (deg < m_) {
            int d = 0;
            for (u64 k = 1; k <= deg; ++k)
                if (!p[k].zero()) d = std::max(d, poly_clog2(k));
            return 1 + d;
        }
        const u64 e = giant_below(deg);
        Poly hi, lo;
        split(p, e, hi, lo);
        const int dh = hi.size() == 1 ? 1 + poly_clog2(e) : 1 + std::max(depth(hi), poly_clog2(e));
        return lo.size() >= 2 ? std::max(dh, depth(lo)) : dh;
    }
    void mark(const Poly &p) // the powers the leaves and the splits use
    {
        const u64 deg = p.size() - 1;
        if (deg < m_) {
            for (u64 k = 1; k <= deg; ++k)
                if (!p[k].zero()) need_[k] = true;
            return;
        }
        const u64 e = giant_below(deg);
        need_[e] = true;
        Poly hi, lo;
        split(p, e, hi, lo);
        if (hi.size() >= 2) mark(hi);
        if (lo.size() >= 2) mark(lo);
    }
    // the power tree: every needed power from its halves, in ascending order
    void build_powers(PolyPlan &pl)
    {
        for (u64 k = 1023; k >= 2; --k)
            if (need_[k]) need_[k / 2] = need_[k - k / 2] = true;
        buf_[1] = add_buf(pl, 0, L_);
        for (u64 k = 2; k < 1024; ++k) {
            if (!need_[k]) continue;
            const u64 f = k / 2, c = k - f;
            const int l = std::min(level_[f], level_[c]);
            if (l < 2) throw std::invalid_argument(w_ + ": the chain is too short for power " + std::to_string(k));
            if (cheb_) {
                cheb_power(pl, k, c, f, l);
                continue;
            }
            const int a = dropped(pl, f, l), b = dropped(pl, c, l);
            level_[k] = l - 1;
            scale_[k] = scale_[f] * scale_[c] / (double)P.primes[l - 1].q;
            buf_[k] = add_buf(pl, 2, l - 1);
            PolyStep s{kPolyMulRelin, l};
            s.a = a; s.b = b; s.dst = buf_[k];
            push(pl, std::move(s));
            ++pl.info.powers;
            pl.info.power_mask[k / 64] |= (u64)1 << (k % 64);
        }
    }
    // eval(p, Lt, S) into `dst` (-1: a new pool buffer); returns the buffer, at level Lt
    int eval(PolyPlan &pl, const Poly &p, int Lt, double S, int dst)
    {
        const u64 deg = p.size() - 1;
        const double T = S * (double)P.primes[Lt].q;
        if (deg < m_) {
            std::vector<LeafTerm> t;
            for (u64 k = 1; k <= deg; ++k)
                if (!p[k].zero()) t.push_back({k, (p[k].re * T) / scale_[k], (p[k].im * T) / scale_[k]});
            return leaf(pl, t, !p[0].zero(), p[0].re * T, p[0].im * T, Lt, dst);
        }
        const u64 e = giant_below(deg);
        Poly hi, lo;
        split(p, e, hi, lo);
        const bool sum = !lo.empty();
        int prod;
        if (hi.size() == 1) {
            prod = leaf(pl, {{e, (hi[0].re * T) / scale_[e], (hi[0].im * T) / scale_[e]}}, false, 0.0, 0.0, Lt, sum ? -1 : dst);
        } else {
            const int H = eval(pl, hi, Lt + 1, T / scale_[e], -1);
            if (level_[e] < Lt + 1) throw std::invalid_argument(w_ + ": a split's power lies below its product's level");
            const int g = dropped(pl, e, Lt + 1);
            prod = sum ? add_buf(pl, 2, Lt) : out_buf(pl, dst, Lt);
            PolyStep s{kPolyMulRelin, Lt + 1};
            s.a = H; s.b = g; s.dst = prod;
            push(pl, std::move(s));
        }
        if (!sum) return prod;
        const int out = out_buf(pl, dst, Lt);
        if (lo.size() == 1) { // a constant: prod * 1 + c_0 S, one combination at the result's level
            PolyStep s{kPolyCombine, Lt};
            s.terms = {prod};
            s.cplx = cplx_;
            s.scalars.assign((size_t)Lt * (cplx_ ? 2 : 1), 1);
            residues(Lt, lo[0].re * S, lo[0].im * S, s.cst);
            s.dst = out;
            push(pl, std::move(s));
            return out;
        }
        const int LO = eval(pl, lo, Lt, S, -1);
        PolyStep s{kPolyAdd, Lt};
        s.a = prod; s.b = LO; s.dst = out;
        push(pl, std::move(s));
        return out;
    }
    u64 words() const { return words_; }
    // the fused steps' row block [nc][2][N], behind everything taken so far; returns its word offset per ciphertext
    u64 take_row_block()
    {
        const u64 at = words_;
        words_ += 2 * (u64)P.N;
        return at;
    }
    // he355_ckks_eval_mod: r steps y <- 2 y^2 - 1 from buffer `y` at level l0 and scale s0; step j squares with the rescale to level
    // l_j = l0 - j, s_j = (s_(j-1) * s_(j-1)) / q[l_j], then ONE combination 2 z - s_j at l_j (the last one into `dst`).  Returns s_r.
    double double_angles(PolyPlan &pl, int y, int l0, double s0, int r, int dst)
    {
        double s = s0;
        for (int j = 1; j <= r; ++j) {
            const int lj = l0 - j;
            s = (s * s) / (double)P.primes[lj].q;
            const int z = add_buf(pl, 2, lj);
            PolyStep m{kPolyMulRelin, lj + 1};
            m.a = y; m.b = y; m.dst = z; m.angle = true;
            push(pl, std::move(m));
            PolyStep c{kPolyCombine, lj};
            c.terms = {z};
            c.scalars.assign((size_t)lj, 2);
            residues(lj, -s, 0.0, c.cst);
            c.dst = y = j == r ? dst : add_buf(pl, 2, lj);
            push(pl, std::move(c));
        }
        return s;
    }

private:
    // T_k = 2 T_a T_b - T_(a-b), a = ceil(k / 2), b = floor(k / 2) at the common level l: the product WITHOUT its rescale, at scale
    // W = s_a * s_b, then ONE fused step 2 P - W (k even: a - b = 0, T_0 = 1 at scale W) or 2 P - (W / s_1) T_1 (k odd: a - b = 1, the
    // input read at its own level L).  T_k lies at level l - 1 with scale s_k = W / q[l - 1].
    void cheb_power(PolyPlan &pl, u64 k, u64 a, u64 b, int l)
    {
        const double W = scale_[a] * scale_[b];
        const int da = dropped(pl, a, l), db = dropped(pl, b, l);
        const int prod = add_buf(pl, 2, l);
        PolyStep m{kPolyMulRelin, l};
        m.a = da; m.b = db; m.dst = prod; m.rescale = false;
        push(pl, std::move(m));
        level_[k] = l - 1;
        scale_[k] = W / (double)P.primes[l - 1].q;
        buf_[k] = add_buf(pl, 2, l - 1);
        PolyStep s{kPolyFused, l};
        s.terms = {prod};
        s.scalars.assign((size_t)l, 2);
        if (k & 1) {
            s.terms.push_back(buf_[1]);
            residues(l, -(W / scale_[1]), 0.0, s.scalars);
        } else {
            residues(l, -W, 0.0, s.cst);
        }
        s.dst = buf_[k];
        push(pl, std::move(s));
        ++pl.info.powers;
        pl.info.power_mask[k / 64] |= (u64)1 << (k % 64);
    }
    int add_buf(PolyPlan &pl, int kind, int L)
    {
        pl.bufs.push_back({kind, kind == 2 ? words_ : 0, L});
        if (kind == 2) words_ += 2 * (u64)L * P.N;
        return (int)pl.bufs.size() - 1;
    }
    int out_buf(PolyPlan &pl, int dst, int L) { return dst >= 0 ? dst : add_buf(pl, 2, L); }
    // power k at level l: itself, or its copy without the rows from l on (made once per level)
    int dropped(PolyPlan &pl, u64 k, int l)
    {
        if (level_[k] == l) return buf_[k];
        const auto key = std::make_pair(k, l);
        const auto it = drops_.find(key);
        if (it != drops_.end()) return it->second;
        const int b = add_buf(pl, 2, l);
        PolyStep s{kPolyDrop, l};
        s.a = buf_[k]; s.dst = b;
        push(pl, std::move(s));
        return drops_[key] = b;
    }
    struct LeafTerm { u64 k; double re, im; }; // (exponent, scalar as doubles; im is read by the complex call alone)
    // the residues of one scalar appended to `to`: [L], or the pair [2][L] of he355_ckks_complex_scalar_residues; mags: |A| (and |B|)
    void residues(int L, double re, double im, std::vector<u64> &to, u128 *mags = nullptr)
    {
        const size_t at = to.size();
        to.resize(at + (size_t)L * (cplx_ ? 2 : 1));
        if (cplx_) {
            cplx_scalar_residues(P, w_, L, re, im, to.data() + at, mags);
            return;
        }
        poly_scalar_residues(P, w_, L, re, to.data() + at);
        if (mags) {
            bool neg;
            poly_scalar_integer(re, mags[0], neg);
            mags[1] = 0;
        }
    }
    // one combination at level Lt + 1 over powers, then the rescale to Lt
    int leaf(PolyPlan &pl, const std::vector<LeafTerm> &t, bool has_const, double cst_re, double cst_im, int Lt, int dst)
    {
        const int Lc = Lt + 1;
        PolyStep s{kPolyCombine, Lc};
        s.cplx = cplx_;
        for (size_t j = 0; j < t.size(); ++j) {
            if (level_[t[j].k] < Lc) throw std::invalid_argument(w_ + ": a leaf's power lies below the leaf's level");
            s.terms.push_back(buf_[t[j].k]);
            u128 mags[2];
            residues(Lc, t[j].re, t[j].im, s.scalars, mags);
            for (u128 mag : mags)
                if (mag) {
                    int bits = 0;
                    while (mag >> (bits + 1)) ++bits;
                    if (pl.info.min_scalar_bits < 0 || bits < pl.info.min_scalar_bits) pl.info.min_scalar_bits = bits;
                }
        }
        if (has_const) residues(Lc, cst_re, cst_im, s.cst);
        if (cheb_) { // the same leaf as ONE he355_combine_scalars_rescale: no slab at Lt + 1
            s.op = kPolyFused;
            const int o = out_buf(pl, dst, Lt);
            s.dst = o;
            push(pl, std::move(s));
            return o;
        }
        const int tmp = add_buf(pl, 2, Lc);
        s.dst = tmp;
        push(pl, std::move(s));
        const int out = out_buf(pl, dst, Lt);
        PolyStep r{kPolyRescale, Lc};
        r.a = tmp; r.dst = out;
        push(pl, std::move(r));
        return out;
    }
    void push(PolyPlan &pl, PolyStep &&s)
    {
        switch (s.op) {
        case kPolyMulRelin: ++pl.info.products; break;
        case kPolyDrop: ++pl.info.drops; break;
        case kPolyCombine: ++pl.info.combinations; break;
        case kPolyRescale: ++pl.info.rescales; break;
        case kPolyAdd: ++pl.info.adds; break;
        case kPolyFused: ++pl.info.rescales; break; // (the Chebyshev plans: `rescales` counts the fused steps)
        }
        pl.steps.push_back(std::move(s));
    }
    const Params &P;
    const std::string w_;
    const int L_;
    const u64 m_;
    const bool cplx_, cheb_;
    bool need_[1024] = {};
    int level_[1024] = {}, buf_[1024] = {};
    double scale_[1024] = {};
    std::map<std::pair<u64, int>, int> drops_;
    u64 words_ = 0;
};

// `chunk`: the context's batch chunk (info.chunks, and the caller's bound of the pool bytes); in / out may be null for a plan alone
// (check_ptrs false: he355_ckks_eval_poly_plan)
// im_coeffs: the imaginary parts of he355_ckks_eval_poly_complex (cplx true; both lists are needed), null for the real call
// basis: kBasisChebyshev -- he355_ckks_eval_chebyshev (cheb_args.h; real coefficients): the powers are T_k, every power and every leaf ends in
// ONE he355_combine_scalars_rescale (kPolyFused), a node splits in the Chebyshev basis; the depth formulas, the node rule and every refusal
// are the monomial call's.  double_angles = r > 0: he355_ckks_eval_mod -- the polynomial at the scale the r steps y <- 2 y^2 - 1 need, then
// those steps; the depth grows by r and info.out_scale is the scale the steps arrive at.
inline PolyPlan plan_eval_poly(const Params &p, const char *what, int L, u64 n, const u64 *in, const double *coeffs, u64 n_coeffs, int log_baby, double in_scale,
                               double out_scale, const u64 *out, bool check_ptrs, u64 chunk, const double *im_coeffs = nullptr, bool cplx = false,
                               int basis = kBasisMonomial, int double_angles = 0)
{
    const std::string w(what);
    if (p.scheme != kSchemeCKKS) throw std::invalid_argument(w + ": polynomial evaluation is a CKKS operation");
    check_level(p, w, L);
    if (p.K < 2) throw std::invalid_argument(w + ": encryption parameters do not support key switching");
    if (n_coeffs > 1024) throw std::invalid_argument(w + ": too many coefficients (at most 1024)");
    if (n_coeffs && (!coeffs || (cplx && !im_coeffs))) throw std::invalid_argument(w + ": null coefficients");
    if (log_baby < 1 || log_baby > 6) throw std::invalid_argument(w + ": log_baby must be 1..6");
    for (u64 k = 0; k < n_coeffs; ++k)
        if (!std::isfinite(coeffs[k]) || (cplx && !std::isfinite(im_coeffs[k]))) throw std::invalid_argument(w + ": coefficient " + std::to_string(k) + " is not finite");
    if (!std::isfinite(in_scale) || !std::isfinite(out_scale) || in_scale <= 0 || out_scale <= 0) throw std::invalid_argument(w + ": a scale must be finite and positive");
    const PolyPlanner::Poly poly = PolyPlanner::trimmed(coeffs, cplx ? im_coeffs : nullptr, n_coeffs);
    if (poly.size() < 2) throw std::invalid_argument(w + ": no non-zero coefficient above c_0 (nothing to evaluate on a ciphertext)");
    PolyPlanner pp(p, w, L, log_baby, in_scale, cplx, basis);
    PolyPlan pl;
    const int pdepth = pp.depth(poly);
    pl.info.depth = pdepth + double_angles;
    pl.info.degree = (int32_t)poly.size() - 1;
    if (pl.info.depth >= L) throw std::invalid_argument(w + ": the evaluation takes " + std::to_string(pl.info.depth) + " levels, the input has " + std::to_string(L) + " (depth must be below L)");
    pl.info.L_out = L - pl.info.depth;
    pl.info.min_scalar_bits = -1;
    pl.info.out_scale = out_scale;
    pp.mark(poly);
    pp.build_powers(pl);
    const int dst = (int)pl.bufs.size();
    pl.bufs.push_back({1, 0, pl.info.L_out});
    if (double_angles > 0) { // S_r = out_scale, S_(j-1) = sqrt(S_j * q[l_j]) backwards; the polynomial runs at the target S_0
        const int l0 = L - pdepth;
        double S = out_scale;
        for (int j = double_angles; j >= 1; --j) S = std::sqrt(S * (double)p.primes[l0 - j].q);
        if (!std::isfinite(S) || S <= 0) throw std::invalid_argument(w + ": a scale must be finite and positive");
        const int y = pp.eval(pl, poly, l0, S, -1);
        pl.info.out_scale = pp.double_angles(pl, y, l0, S, double_angles, dst);
        pl.info.reserved[0] = (u64)double_angles;
    } else {
        pp.eval(pl, poly, pl.info.L_out, out_scale, dst);
    }
    if (basis == kBasisChebyshev) pl.row_off = pp.take_row_block();
    pl.words_per_ct = pp.words();
    const u128 cap = (u128)1 << 60, in_w = (u128)n * 2 * (u128)L * p.N, out_w = (u128)n * 2 * (u128)pl.info.L_out * p.N;
    if (n > cap || in_w > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    pl.empty = n == 0;
    const u64 c = std::min<u64>(chunk ? chunk : 1, n);
    pl.info.chunks = c ? (n + c - 1) / c : 0;
    if (pl.empty || !check_ptrs) return pl;
    if (!in || !out) throw std::invalid_argument(w + ": null ciphertexts");
    if (word_range(w, out, (u64)out_w).overlaps(word_range(w, in, (u64)in_w))) throw std::invalid_argument(w + ": `d_out` overlaps `d_in`");
    return pl;
}

} // namespace he355
