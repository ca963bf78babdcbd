// sim_bfv_seeded.cpp -- TEST-ONLY.  Runs the arithmetic of seeded BFV queries and Galois keys (csrc/bfv_seeded_core.h: the very functions the
// HIP kernels k_bfv_seeded_gen and k_bfv_seeded_finish compile -- the uniform draw with its hoisted base word, host-made limit and Barrett
// reduction, the error draw, the client's finish step) and the samplers and stream functions of csrc/client/sampler.h on the CPU, so that
// tests/test_bfv_seeded_core_cpu.py and tests/test_bfv_seeded_ref_cpu.py can hold them to Python integers without a GPU.  Built into
// tests/csim/_build; the product never contains it.
#include "../../reference-seal-backend_amd/csrc/bfv_seeded_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

extern "C" {

// ---- client/sampler.h as it stands --------------------------------------------------------------------------------------------------------
void sim_seeded_sampler_uniform(uint64_t seed, uint64_t stream, const uint64_t *ns, uint64_t count, uint64_t q, uint64_t *out)
{
    for (uint64_t k = 0; k < count; ++k) out[k] = client::sample_uniform_at(seed, stream, ns[k], q);
}
void sim_seeded_sampler_cbd(uint64_t seed, uint64_t stream, const uint64_t *ns, uint64_t count, int32_t *out)
{
    for (uint64_t k = 0; k < count; ++k) out[k] = client::sample_cbd_at(seed, stream, ns[k]);
}
uint64_t sim_seeded_word(uint64_t seed, uint64_t stream, uint64_t n) { return client::sample_word(seed, stream, n); }
uint64_t sim_seeded_a_stream(uint64_t r, uint64_t i) { return client::seeded_a_stream(r, i); }
uint64_t sim_seeded_e_stream(uint64_t r) { return client::seeded_e_stream(r); }
uint64_t sim_seeded_enc_stream(uint64_t r, int which) { return client::enc_stream(r, which); }
uint64_t sim_seeded_keygen_stream(uint64_t key_id, uint64_t digit, uint64_t K, uint64_t which) { return client::keygen_stream(key_id, digit, K, which); }
uint64_t sim_seeded_max_index(void) { return kBfvSeededMaxIndex; }

// ---- bfv_seeded_core.h ----------------------------------------------------------------------------------------------------------------------
uint64_t sim_seeded_limit(uint64_t q) { return bfv_seeded_limit(q); }
// the kernel's draw at coefficients ns[.]: base word once, then bfv_seeded_uniform with make_mod's Barrett words
void sim_seeded_uniform(uint64_t seed, uint64_t stream, const uint64_t *ns, uint64_t count, uint64_t q, uint64_t *out)
{
    const ModU64 m = make_mod(q);
    const u64 base = bfv_seeded_base(seed, stream), lim = bfv_seeded_limit(q);
    for (uint64_t k = 0; k < count; ++k) out[k] = bfv_seeded_uniform(base, ns[k], lim, m);
}
void sim_seeded_error(uint64_t seed, uint64_t stream, const uint64_t *ns, uint64_t count, int32_t *out)
{
    const u64 base = bfv_seeded_base(seed, stream);
    for (uint64_t k = 0; k < count; ++k) out[k] = bfv_seeded_error(base, ns[k]);
}
// barrett64 on any 64-bit word: the reduction the draw ends with
uint64_t sim_seeded_reduce(uint64_t v, uint64_t q) { return barrett64(v, make_mod(q)); }
uint64_t sim_seeded_finish(uint64_t delta, int e, uint64_t w, uint64_t q) { return bfv_seeded_finish(delta, e, w, q); }
// Delta_L(m) mod q_i as the finish kernel forms it (bfv_level_core.h), q: the L primes of the level
uint64_t sim_seeded_delta(const uint64_t *q, int L, uint64_t t, uint64_t m, int i)
{
    const BfvDeltaConst dc = bfv_delta_const(q, L, t);
    return bfv_delta_residue(m, bfv_delta_fix(m, dc), dc.qdivt[i], make_mod(q[i]));
}

} // extern "C"
