// bfv_seeded_core.h -- the per-coefficient arithmetic of seeded (secret-key) BFV queries and seeded Galois keys: the uniform half of a
// ciphertext or key drawn from a PUBLIC seed, and the client's c0 = Delta(m) - e - a s.  Host-compilable on purpose, like the other *_core.h:
// the HIP kernels (he355_kernels_bfv_seeded.hip: k_bfv_seeded_gen, k_bfv_seeded_finish) and the test-only simulator
// (tests/csim/sim_bfv_seeded.cpp, which holds these very functions to client/sampler.h and to Python integers on the CPU, in both builds of
// the u64 engine) compile the same text.  The definition is include/he355.h's "Seeded BFV queries and Galois keys".
//
//   uniform : client::sample_uniform_at(seed, stream, n, q) with its pieces hoisted: the stream's base word (two splitmix64, the same for
//             every coefficient of a polynomial), the acceptance limit of q (host-made: it needs a division) and the final v mod q as
//             modarith.h's barrett64, which is exact for every 64-bit v -- no 64-bit division runs on the device.  The first draw goes
//             down a straight path; draws 2..8 sit in a branch taken with probability (2^64 mod q) / 2^64, below 2^-4 for every q < 2^60.
//   finish  : c0 = (Delta(m) - e - w) mod q_i with w = iNTT(a (.) s), e the centred binomial error of the ciphertext's own stream.
#pragma once
#include <stddef.h>

#include "bfv_level_core.h"
#include "client/sampler.h"

namespace he355 {

constexpr u64 kBfvSeededMaxIndex = (u64)1 << 40; // first_index + n may not pass it: the streams of client/sampler.h stay apart below it

// sample_word(seed, stream, n) = splitmix64(base + n): the part of it that does not depend on n
HE_HD u64 bfv_seeded_base(u64 seed, u64 stream) { return client::splitmix64(seed ^ client::splitmix64(stream)); }
// the largest accepted draw under q (sample_uniform_at's `lim`).  Host side: the kernels take it as an argument
inline u64 bfv_seeded_limit(u64 q) { return ~(u64)0 - (~(u64)0 % q) - 1; }
// coefficient n of the uniform polynomial of the stream behind `base`, in [0, q)
HE_HD u64 bfv_seeded_uniform(u64 base, u64 n, u64 lim, const ModU64 &m)
{
    u64 v = client::splitmix64(base + 8 * n);
    if (v > lim) { // rare: the sub-counters 8n + 1 .. 8n + 7, the last one kept whatever it is
        for (int k = 1; k < 8; ++k) {
            v = client::splitmix64(base + 8 * n + (u64)k);
            if (v <= lim) break;
        }
    }
    return barrett64(v, m);
}
// the centred binomial error of the stream behind `base` at coefficient n (client::sample_cbd_at)
HE_HD int bfv_seeded_error(u64 base, u64 n)
{
    const u64 w = client::splitmix64(base + n);
    return client::popcount21(w) - client::popcount21(w >> 21);
}
// c0 = (delta - e - w) mod q: delta = Delta_L(m) mod q (0 for the seeded zero), |e| <= 21, w < q
HE_HD u64 bfv_seeded_finish(u64 delta, int e, u64 w, u64 q) { return submod(submod(delta, client::small_to_residue(e, q), q), w, q); }

} // namespace he355
