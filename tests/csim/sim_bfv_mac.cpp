// sim_bfv_mac.cpp -- TEST-ONLY.  Runs the product's per-coefficient arithmetic of the NTT-form BFV plaintext inner product
// (csrc/bfv_mac_core.h: the very functions the HIP kernel k_bfv_plain_mac compiles -- the 128-bit multiply-add, the run-length rule, the
// reduction -- and the loop that cuts a sum into runs) on the CPU, with the Barrett constants the product builds (Params), so that
// tests/test_bfv_mac_core_cpu.py can hold it to Python integers without a GPU.  The arithmetic does not depend on the form of the u64
// engine: the tests load the Shoup library.  Built into tests/csim/_build; the product never contains it.
#include <stdexcept>
#include <vector>

#include "../../reference-seal-backend_amd/csrc/bfv_mac_core.h"
#include "../../reference-seal-backend_amd/csrc/he_params.h"

using namespace he355;

namespace {
struct MacSim {
    Params *p = nullptr;
};
} // namespace

extern "C" {

// a BFV context's key chain (every prime of it, the special one included); null when the parameters are refused
void *sim_bfvmac_create(size_t N, const int *bits, size_t n_bits, int plain_bits)
{
    try {
        MacSim *s = new MacSim();
        s->p = Params::create(kSchemeBFV, N, std::vector<int>(bits, bits + n_bits), plain_bits, false);
        return s;
    } catch (const std::exception &) {
        return nullptr;
    }
}
// the same over explicit moduli (primes whose run length the prime-size rule never produces)
void *sim_bfvmac_create_primes(size_t N, const uint64_t *primes, size_t n, uint64_t plain_modulus)
{
    try {
        MacSim *s = new MacSim();
        s->p = Params::create_primes(kSchemeBFV, N, std::vector<u64>(primes, primes + n), plain_modulus, false);
        return s;
    } catch (const std::exception &) {
        return nullptr;
    }
}
void sim_bfvmac_destroy(void *h)
{
    MacSim *s = static_cast<MacSim *>(h);
    if (s) { delete s->p; delete s; }
}
size_t sim_bfvmac_primes(void *h) { return static_cast<MacSim *>(h)->p->K; }
uint64_t sim_bfvmac_q(void *h, size_t i) { return static_cast<MacSim *>(h)->p->primes[i].q; }
// the rule: terms one 128-bit sum takes under q, and the cap it states
uint64_t sim_bfvmac_run(uint64_t q) { return bfv_mac_run(q); }
uint64_t sim_bfvmac_max_run(void) { return kBfvMacMaxRun; }
// out[c] = sum_k a[k][c] b[k][c] mod q_i, c < n, as one accumulator of the kernel computes it: a, b [inner][n] canonical residues.
// run == 0: the rule's own value.  peak (optional, [2]): the largest 128-bit sum any coefficient reached before a reduction, low / high word
int sim_bfvmac_dot(void *h, size_t i, const uint64_t *a, const uint64_t *b, uint64_t inner, size_t n, uint64_t run, uint64_t *out, uint64_t *peak)
{
    MacSim *s = static_cast<MacSim *>(h);
    if (i >= s->p->K) return 1;
    const ModU64 m = s->p->primes[i].mod;
    if (!run) run = bfv_mac_run(m.q);
    if (run < 2) return 2;
    for (size_t c = 0; c < n; ++c) out[c] = bfv_mac_dot(a + c, n, b + c, n, inner, run, m);
    if (peak) { // the same cuts, watching the sum (checked arithmetic: a wrap would show as a sum smaller than the one before)
        u128 top = 0;
        for (size_t c = 0; c < n; ++c) {
            u128 acc = 0;
            u64 k = 0, take = run;
            while (k < inner) {
                const u64 end = inner - k < take ? inner : k + take;
                for (; k < end; ++k) {
                    const u128 before = acc;
                    bfv_mac_add(acc, a[k * n + c], b[k * n + c]);
                    if (acc < before) return 3; // left 128 bits
                }
                if (acc > top) top = acc;
                if (k < inner) bfv_mac_fold(acc, m);
                take = run - 1;
            }
        }
        peak[0] = (u64)top; peak[1] = (u64)(top >> 64);
    }
    return 0;
}

} // extern "C"
