// hoist_args.h -- the argument checks of the hoisted rotations (he355_apply_galois_hoisted, he355_rotate_hoisted,
// he355_rotate_hoisted_plain_sum, he355_rotate_hoisted_plain_sum_lazy, he355_plain_extend_special) that need no device, made ONCE per call in the style of bfv_pir_args.h: the C ABI wrapper runs the check
// before it asks for a device -- a refusal is HE355_E_INVALID_ARGS whether a device exists or not -- and hands the elements the check worked
// out to DeviceContext.  Whether an element's Galois key is installed is the device context's to know; it checks that before its first launch.
// Host-only on purpose: no HIP header, so tests/rotate_hoisted_args_main.cpp runs every check at its edges under the sanitizers.
#pragma once
#include <vector>

#include "bfv_pir_args.h"

namespace he355 {

// elts: the Galois element of every output block, 1 = the identity (a copy; no key); keyed: how many are not the identity
struct HoistPlan {
    std::vector<uint32_t> elts;
    u64 keyed = 0;
    bool empty = false; // n == 0 or no elements: the call touches nothing
};
// `in` [n][2][L][N]; `out` [n_elts][n][2][L][N], or with `plain_sum` [n][2][L][N] and `plain` [n_elts][L][N].  The elements come from
// h_elts, or from h_steps (step 0: the identity; any other step through Params::galois_elt_from_step) when h_elts is null.
// plain_special (he355_rotate_hoisted_plain_sum_lazy): every plaintext carries one more row, under the special prime: [n_elts][L + 1][N].
inline HoistPlan plan_rotate_hoisted(const Params &p, const char *what, int L, int ntt_form, u64 n, const u64 *in, const uint32_t *h_elts, const int32_t *h_steps,
                                     u64 n_elts, const u64 *plain, const u64 *out, bool plain_sum, bool plain_special = false)
{
    const std::string w(what);
    check_level(p, w, L);
    if (p.K < 2) throw std::invalid_argument(w + ": encryption parameters do not support key switching");
    if (ntt_form != 0 && ntt_form != 1) throw std::invalid_argument(w + ": ntt_form must be 0 or 1");
    if (ntt_form == 0 && p.scheme != kSchemeBFV) throw std::invalid_argument(w + ": CKKS ciphertexts are in NTT form (ntt_form must be 1)");
    HoistPlan pl;
    if (n_elts && !h_elts && !h_steps) throw std::invalid_argument(w + (plain_sum || h_steps ? ": null steps" : ": null elements"));
    if (n_elts > ((u64)1 << 20)) throw std::invalid_argument(w + ": too many elements for one call (at most 2^20)");
    pl.elts.reserve((size_t)n_elts);
    for (u64 r = 0; r < n_elts; ++r) {
        uint32_t e;
        if (h_elts) {
            e = h_elts[r];
            if (!(e & 1) || e >= 2 * p.N) throw std::invalid_argument(w + ": Galois element " + std::to_string(e) + " is not valid (odd, below 2N)");
        } else {
            const int32_t s = h_steps[r];
            e = s == 0 ? 1 : p.galois_elt_from_step(s);
            if (!e) throw std::invalid_argument(w + ": step " + std::to_string(s) + " has no Galois element (|step| must be below N / 2)");
        }
        pl.elts.push_back(e);
        pl.keyed += e != 1;
    }
    // every slab in words, formed in 128 bits: 2^60 words (2^63 bytes) is the most one may span
    const u128 ctn = (u128)2 * (u128)L * p.N, in_w = (u128)n * ctn, out_w = plain_sum ? in_w : in_w * n_elts, plain_w = plain_sum ? (u128)n_elts * (u128)(L + (plain_special ? 1 : 0)) * p.N : 0;
    const u128 cap = (u128)1 << 60;
    if (n > cap || in_w > cap || out_w > cap || plain_w > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    pl.empty = n == 0 || n_elts == 0;
    if (pl.empty) return pl;
    const AddrRange ri = word_range(w, in, (u64)in_w), ro = word_range(w, out, (u64)out_w);
    if (ro.overlaps(ri)) throw std::invalid_argument(w + ": `d_out` overlaps `d_in`");
    if (plain_sum) {
        if (!plain) throw std::invalid_argument(w + ": null plaintexts");
        if (ro.overlaps(word_range(w, plain, (u64)plain_w))) throw std::invalid_argument(w + (plain_special ? ": `d_out` overlaps `d_plain_qp`" : ": `d_out` overlaps `d_plain`"));
    }
    return pl;
}
// he355_plain_extend_special: plain_ntt [n][L][N] -> plain_qp [n][L + 1][N].  True: n == 0, the call touches nothing.
inline bool plan_plain_extend(const Params &p, int L, u64 n, const u64 *plain_ntt, const u64 *plain_qp)
{
    const std::string w("he355_plain_extend_special");
    check_level(p, w, L);
    if (p.K < 2) throw std::invalid_argument(w + ": encryption parameters have no special prime");
    const u128 in_w = (u128)n * (u128)L * p.N, out_w = (u128)n * (u128)(L + 1) * p.N, cap = (u128)1 << 60;
    if (n > cap || in_w > cap || out_w > cap) throw std::invalid_argument(w + ": the plaintexts span more than 2^60 words");
    if (n == 0) return true;
    if (!plain_ntt || !plain_qp) throw std::invalid_argument(w + ": null pointer");
    if (word_range(w, plain_qp, (u64)out_w).overlaps(word_range(w, plain_ntt, (u64)in_w))) throw std::invalid_argument(w + ": `d_plain_qp` overlaps `d_plain_ntt`");
    return false;
}

} // namespace he355
