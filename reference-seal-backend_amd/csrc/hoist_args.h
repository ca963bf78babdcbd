// hoist_args.h -- the argument checks of the hoisted rotations (he355_apply_galois_hoisted, he355_rotate_hoisted,
// he355_rotate_hoisted_plain_sum, he355_rotate_hoisted_plain_sum_lazy, he355_linear_transform_bsgs, he355_plain_extend_special) that need no device, made ONCE per call in the style of bfv_pir_args.h: the C ABI wrapper runs the check
// before it asks for a device -- a refusal is HE355_E_INVALID_ARGS whether a device exists or not -- and keeps the elements the check worked
// out as the plan of the C ABI function (hoisted_rotations.inc).  Whether an element's Galois key is installed is the device context's to know; it checks that before its first launch.
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
// he355_linear_transform_bsgs: out[c] = sum_j rot_{G_j}(sum_i plain[j][i] (.) rot_{b_i}(in[c])).  `in`, `out` [n][2][L][N]; plain
// [n_giant][n_baby][L + 1][N]; mask [n_giant][n_baby] bytes or null (all terms).  A step is USED when a term that is not masked names it:
// only used keyed steps need their Galois keys (the device context's to check).
struct BsgsPlan {
    std::vector<uint32_t> baby, giant;    // the Galois element of every step, 1 = the identity
    std::vector<int> slot;                // per baby: its slot in the baby store, -1: not used
    std::vector<u64> row_first;           // per giant row: its first entry in `terms` (n_giant + 1 entries); an empty range: the row is not used
    std::vector<uint32_t> terms;          // per used term, row by row: (slot of the baby, index of the plaintext in the row) -- two words each
    u64 slots = 0, keyed_babies = 0, keyed_rows = 0, used_rows = 0; // used ones only
    bool empty = false;                   // n == 0, n_baby == 0 or n_giant == 0: the call touches nothing
};
inline BsgsPlan plan_linear_transform_bsgs(const Params &p, int L, u64 n, const u64 *in, const int32_t *h_baby, u64 n_baby, const int32_t *h_giant, u64 n_giant,
                                           const u64 *plain_qp, const uint8_t *h_mask, const u64 *out)
{
    const std::string w("he355_linear_transform_bsgs");
    check_level(p, w, L);
    if (p.K < 2) throw std::invalid_argument(w + ": encryption parameters do not support key switching");
    BsgsPlan pl;
    if ((n_baby && !h_baby) || (n_giant && !h_giant)) throw std::invalid_argument(w + ": null steps");
    const u128 pairs = (u128)n_baby * n_giant;
    if (pairs > ((u128)1 << 20)) throw std::invalid_argument(w + ": too many (giant, baby) pairs for one call (at most 2^20)");
    auto elts = [&](const int32_t *steps, u64 count, std::vector<uint32_t> &to) {
        to.reserve((size_t)count);
        for (u64 r = 0; r < count; ++r) {
            const int32_t s = steps[r];
            const uint32_t e = s == 0 ? 1 : p.galois_elt_from_step(s);
            if (!e) throw std::invalid_argument(w + ": step " + std::to_string(s) + " has no Galois element (|step| must be below N / 2)");
            to.push_back(e);
        }
    };
    if (pairs) { // (with one list empty the other may be longer than 2^20: nothing is read of it)
        elts(h_baby, n_baby, pl.baby);
        elts(h_giant, n_giant, pl.giant);
    }
    // every slab in words, formed in 128 bits: 2^60 words (2^63 bytes) is the most one may span
    const u128 in_w = (u128)n * 2 * (u128)L * p.N, plain_w = pairs * (u128)(L + 1) * p.N, cap = (u128)1 << 60;
    if (n > cap || in_w > cap || plain_w > cap) throw std::invalid_argument(w + ": the ciphertexts span more than 2^60 words");
    pl.empty = n == 0 || pairs == 0;
    if (pl.empty) return pl;
    pl.slot.assign((size_t)n_baby, -1);
    pl.row_first.assign((size_t)n_giant + 1, 0);
    for (u64 j = 0; j < n_giant; ++j) { // slots in the order of first use, which is the order of the baby list
        for (u64 i = 0; i < n_baby; ++i)
            if (!h_mask || h_mask[j * n_baby + i]) pl.slot[(size_t)i] = 0;
    }
    for (u64 i = 0; i < n_baby; ++i)
        if (pl.slot[(size_t)i] == 0) {
            pl.slot[(size_t)i] = (int)pl.slots++;
            pl.keyed_babies += pl.baby[(size_t)i] != 1;
        }
    for (u64 j = 0; j < n_giant; ++j) {
        pl.row_first[(size_t)j] = pl.terms.size() / 2;
        for (u64 i = 0; i < n_baby; ++i)
            if (!h_mask || h_mask[j * n_baby + i]) {
                pl.terms.push_back((uint32_t)pl.slot[(size_t)i]);
                pl.terms.push_back((uint32_t)i);
            }
        if (pl.terms.size() / 2 > pl.row_first[(size_t)j]) {
            ++pl.used_rows;
            pl.keyed_rows += pl.giant[(size_t)j] != 1;
        }
    }
    pl.row_first[(size_t)n_giant] = pl.terms.size() / 2;
    if (pl.terms.empty()) throw std::invalid_argument(w + ": the mask sets no term");
    if (!plain_qp) throw std::invalid_argument(w + ": null plaintexts");
    if (!in || !out) throw std::invalid_argument(w + ": null ciphertexts");
    const AddrRange ri = word_range(w, in, (u64)in_w), ro = word_range(w, out, (u64)in_w);
    if (ro.overlaps(ri)) throw std::invalid_argument(w + ": `d_out` overlaps `d_in`");
    if (ro.overlaps(word_range(w, plain_qp, (u64)plain_w))) throw std::invalid_argument(w + ": `d_out` overlaps `d_plain_qp`");
    return pl;
}
// What he355_linear_transform_bsgs takes from the pool at a chunk of `c` ciphertexts: the baby store, [slots][c][2][L + 1][N], and the two
// Q P blocks (the inner sum of a keyed giant row; the giant accumulator), [c][2][L][N] + [c][2][N] each.  Raw bytes:
// DevicePool::alloc rounds a request to its size class itself (device_pool.h, which needs HIP and is not included here).
inline size_t bsgs_block_bytes(size_t c, int L, size_t N) { return c * 2 * (size_t)(L + 1) * N * 8; }
inline size_t bsgs_store_bytes(size_t slots, size_t c, int L, size_t N) { return slots * c * 2 * (size_t)(L + 1) * N * 8; }
// he355_linear_transform_bsgs_scratch_bytes: the most a call with n_baby baby steps takes from the pool -- every baby used, the chunk the
// batch chunk (chunk_ops may only shorten it).  0 where the call does nothing or is refused (more than 2^20 babies are more than 2^20
// pairs); formed in 128 bits and saturated, so a huge batch cannot wrap into a small bound.
inline u64 bsgs_scratch_bytes(size_t chunk, const Params &p, int L, u64 n, u64 n_baby)
{
    const u64 c = std::min<u64>(chunk, n);
    if (!c || !n_baby || n_baby > ((u64)1 << 20)) return 0;
    const u128 block = (u128)c * 2 * (u128)(L + 1) * p.N * 8, cls = (u128)2 << 20; // (above 16 MiB the classes are multiples of 2 MiB: one more covers any rounding)
    const u128 total = (u128)n_baby * block + cls + 2 * (block + cls);
    return total > ~(u64)0 ? ~(u64)0 : (u64)total;
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
