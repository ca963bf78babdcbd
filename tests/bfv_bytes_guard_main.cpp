// bfv_bytes_guard_main.cpp -- TEST-ONLY, stand-alone.  Holds the PIR database codec (csrc/bfv_bytes_core.h) to its rule that no word past the
// one that holds the last valid byte is read, and none before the one that holds the first: every byte slab is placed at the very END of a
// heap block whose size is rounded up to 8 (and, for a non-zero offset, begins `off` bytes into the block's first word), so that a read of
// the next aligned word is a heap overflow the address sanitizer reports.  tests/test_bfv_bytes_core_cpu.py compiles this file with
// -fsanitize=address,undefined and runs it as a child process: exit status 0 means every (w, offset, B) of the grid passed, values included.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../reference-seal-backend_amd/csrc/bfv_bytes_core.h"

using namespace he355;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
// bit b of the B-byte little-endian integer
static int bit_of(const unsigned char *p, uint64_t B, uint64_t b) { return b < 8 * B ? (p[b >> 3] >> (b & 7)) & 1 : 0; }

static int run(uint64_t N, int w, unsigned off, uint64_t B)
{
    // the block: `off` filler bytes, B bytes of data, and nothing after them but what rounds the size up to 8
    const size_t size = (off + B + 7) / 8 * 8;
    unsigned char *block = static_cast<unsigned char *>(std::aligned_alloc(8, size));
    std::memset(block, 0xFF, size);
    unsigned char *data = block + off;
    for (uint64_t i = 0; i < B; ++i) data[i] = (unsigned char)rnd();
    if (B > 1) data[B - 1] |= 0x80; // the top bit of the last byte is set: it must show
    std::vector<uint64_t> coef(N), junk(N);
    const BfvByteSrc s = bfv_bytes_src(data, B);
    int bad = 0;
    for (uint64_t e = 0; e < N; ++e) {
        coef[e] = bfv_bytes_field(s, e, w);
        uint64_t want = 0;
        for (int b = 0; b < w; ++b) want |= (uint64_t)bit_of(data, B, e * w + b) << b;
        if (coef[e] != want) ++bad;
        junk[e] = coef[e] | (rnd() << w); // pack masks what lies above bit w
    }
    // pack into a block of exactly ceil(B / 8) words
    const uint64_t W = bfv_bytes_words(B);
    uint64_t *packed = static_cast<uint64_t *>(std::aligned_alloc(8, W * 8));
    for (uint64_t k = 0; k < W; ++k) packed[k] = bfv_bytes_pack_word(junk.data(), N, k, B, w);
    const unsigned char *pb = reinterpret_cast<const unsigned char *>(packed);
    if (std::memcmp(pb, data, B) != 0) ++bad;
    for (uint64_t i = B; i < 8 * W; ++i) bad += pb[i] != 0;
    if (bad) std::fprintf(stderr, "bfv_bytes guard: N %llu w %d offset %u B %llu: %d mismatches\n", (unsigned long long)N, w, off, (unsigned long long)B, bad);
    std::free(packed);
    std::free(block);
    return bad;
}

int main()
{
    int bad = 0;
    for (uint64_t N : {(uint64_t)64, (uint64_t)1024})
        for (int w = 1; w <= 63; ++w) {
            const uint64_t Bmax = bfv_bytes_max(N, w);
            for (unsigned off = 0; off < 8; ++off)
                for (uint64_t B : {(uint64_t)1, (uint64_t)7, (uint64_t)8, (uint64_t)9, Bmax - 1, Bmax})
                    if (B >= 1 && B <= Bmax) bad += run(N, w, off, B);
        }
    if (bad) return 1;
    std::puts("bfv_bytes guard ok");
    return 0;
}
