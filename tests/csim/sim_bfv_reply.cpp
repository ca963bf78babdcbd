// sim_bfv_reply.cpp -- TEST-ONLY.  Runs the arithmetic of BFV reply compression (csrc/bfv_reply_core.h: the very functions the HIP kernels
// k_bfv_reply_pack, k_bfv_reply_lift and k_bfv_reply_finish compile -- the switch to 2^k, one packed output word, a field cut out of whole
// words, the centred lift, the final rounding with its residue) on the CPU, so that tests/test_bfv_reply_core_cpu.py can hold them to Python
// integers without a GPU.  Built into tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/bfv_reply_core.h"

using namespace he355;

extern "C" {

int sim_bfvreply_widths_ok(uint64_t N, uint64_t q, int k0, int k1) { return bfv_reply_widths_ok(N, q, k0, k1) ? 1 : 0; }
uint64_t sim_bfvreply_size(uint64_t N, int k0, int k1) { return bfv_reply_size(N, k0, k1); }
void sim_bfvreply_safe(uint64_t N, uint64_t t, int *k0, int *k1) { bfv_reply_safe(N, t, *k0, *k1); }
// floor(p / k) as the word rule forms it
uint32_t sim_bfvreply_div(uint32_t p, int k) { return bfv_reply_div(p, bfv_reply_cut_of(((uint64_t)1 << 62) + 1, k)); }
// out[i] = cut_k(x[i]) under q
void sim_bfvreply_cut(const uint64_t *x, uint64_t n, int k, uint64_t q, uint64_t *out)
{
    const BfvReplyCut c = bfv_reply_cut_of(q, k);
    for (uint64_t i = 0; i < n; ++i) out[i] = bfv_reply_cut(x[i], c);
}
// the N k / 64 words of one half from its N residues
void sim_bfvreply_pack(const uint64_t *coef, uint64_t N, int k, uint64_t q, uint64_t *words)
{
    const BfvReplyCut c = bfv_reply_cut_of(q, k);
    for (uint64_t j = 0; j < bfv_reply_half_words(N, k); ++j) words[j] = bfv_reply_pack_word(coef, (u32)j, c);
}
// the N fields of one half from its words
void sim_bfvreply_unpack(const uint64_t *words, uint64_t N, int k, uint64_t *out)
{
    for (uint64_t e = 0; e < N; ++e) out[e] = bfv_reply_field(words, (u32)e, k);
}
uint64_t sim_bfvreply_lift(uint64_t y1, int k1, uint64_t q) { return bfv_reply_lift(y1, k1, q); }
// the plaintext coefficient; *bits = the bit length of the residue
uint64_t sim_bfvreply_round(uint64_t y0, uint64_t w, int k0, int k1, uint64_t q, uint64_t t, int *bits)
{
    const BfvReplyCoef c = bfv_reply_round(y0, w, k0, k1, q, t);
    *bits = c.bits;
    return c.m;
}

} // extern "C"
