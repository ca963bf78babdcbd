// rotation_plan_main.cpp -- TEST-ONLY, stand-alone.  Runs rotation_terms and rotation_trie of csrc/rotation_plan.h (the host rule behind
// he355_rotate, he355_rotate_add, he355_rotate_sum and he355_rotate_each) at accepted and refused edges -- steps of 0, at and past +-N/2, at the
// ends of int; every step of a small ring under the power-of-two key set; a one-term NAF without its key; a several-term step that lacks its first,
// a middle or its last term's key; a step whose own key is there while its terms' are not; tries with repeated steps, steps of 0, two steps of one
// element, no steps at all and the 127-step family of the BFV matrix product -- compiled with -fsanitize=address,undefined
// (tests/test_rotation_plan_cpu.py).  The rule negates and shifts step counts the caller chose and indexes its trie by what it finds: none of it
// may overflow a signed type or reach outside a vector.  Prints "rotation_plan ok" and exits 0, or names the first case that went the other way.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <vector>

#include "../reference-seal-backend_amd/csrc/rotation_plan.h"
#include "args_main_common.h"

using namespace he355;

static void must(bool ok, const char *what)
{
    if (!ok) throw std::invalid_argument(std::string("wrong plan: ") + what);
}

int main()
{
    for (size_t N : {(size_t)1024, (size_t)8192}) {
        std::unique_ptr<Params> pp(Params::create(kSchemeCKKS, N, {50, 50}, 0, false));
        const Params &P = *pp;
        const int half = (int)(N / 2);
        auto key_set = [&](std::initializer_list<int> steps) {
            std::set<uint32_t> s;
            for (int t : steps) s.insert(P.galois_elt_from_step(t));
            return s;
        };
        std::set<uint32_t> pow2;
        for (int k = 0; (1 << k) < half; ++k) { pow2.insert(P.galois_elt_from_step(1 << k)); pow2.insert(P.galois_elt_from_step(-(1 << k))); }
        auto terms = [&](int step, const std::set<uint32_t> &keys) { return rotation_terms(P, step, [&](uint32_t e) { return keys.count(e) != 0; }); };
        auto trie = [&](const std::vector<int> &steps, const std::set<uint32_t> &keys) {
            return rotation_trie(P, steps.data(), (u64)steps.size(), [&](uint32_t e) { return keys.count(e) != 0; });
        };
        // steps
        GOOD("step 0", must(terms(0, {}).empty(), "step 0 has no term"));
        for (int s : {half, -half, half + 1, (int)N, 0x7fffffff, (int)0x80000000, (int)0x80000001}) BAD("step too large", terms(s, pow2));
        for (int s = -(half - 1); s < half; ++s) { // every step: the terms add up to the step, up to a whole row
            GOOD("every step", long sum = 0; for (int t : terms(s, pow2)) sum += t; must((sum - s) % half == 0, "the terms do not add up to the step"));
        }
        GOOD("a term of N / 2 is dropped", const std::vector<int> t = terms(half - 3, pow2); must(t == std::vector<int>({1, -4}), "N / 2 - 3"));
        GOOD("a term of -N / 2 is dropped", const std::vector<int> t = terms(-(half - 3), pow2); must(t == std::vector<int>({-1, 4}), "-(N / 2 - 3)"));
        GOOD("N / 2 - 1 is the element of -1", const std::vector<int> t = terms(half - 1, pow2); must(t.size() == 1 && t[0] == half - 1, "N / 2 - 1"));
        GOOD("N / 4", const std::vector<int> t = terms(half / 2, pow2); must(t.size() == 1 && t[0] == half / 2, "N / 4"));
        // keys
        BAD("one-term NAF without its key", terms(8, key_set({1, 2, 4, -1})));
        BAD("one-term NAF without its key", terms(-8, key_set({1, 2, 4, -1})));
        BAD("no keys at all", terms(5, {}));
        GOOD("11 = -1 - 4 + 16", const std::vector<int> t = terms(11, key_set({-1, -4, 16})); must(t == std::vector<int>({-1, -4, 16}), "11"));
        BAD("11 without its first term's key", terms(11, key_set({-4, 16})));
        BAD("11 without a middle term's key", terms(11, key_set({-1, 16})));
        BAD("11 without its last term's key", terms(11, key_set({-1, -4})));
        GOOD("own key, terms without", const std::vector<int> t = terms(11, key_set({11})); must(t.size() == 1 && t[0] == 11, "own key"));
        GOOD("own key through the row length", const std::vector<int> t = terms(3 - half, key_set({3})); must(t.size() == 1 && t[0] == 3 - half, "own key"));
        // tries
        GOOD("no steps", const RotTrie t = trie({}, {}); must(t.nodes.size() == 1 && t.depth() == 0 && t.widest == 1 && t.levels[0].size() == 1, "empty trie"));
        GOOD("steps of 0", const RotTrie t = trie({0, 0, 0}, {}); must(t.nodes.size() == 1 && t.nodes[0].ends == 3, "steps of 0"));
        GOOD("1, 2, 3", const RotTrie t = trie({1, 2, 3}, key_set({1, 2, 4, -1}));
             must(t.nodes.size() == 5 && t.depth() == 2 && t.widest == 3 && t.levels[1].size() == 3 && t.levels[2].size() == 1, "1, 2, 3");
             must(t.nodes[4].parent == 3 && t.nodes[4].pos == 0 && t.nodes[3].kids.size() == 1 && t.nodes[3].ends == 0, "4 under -1"));
        GOOD("repeats", const RotTrie t = trie({3, 3, 0, 1, 0, 3}, key_set({1, 2, 4, -1})); must(t.nodes.size() == 4 && t.nodes[0].ends == 2 && t.nodes[2].ends == 3, "repeats"));
        GOOD("one element twice", const RotTrie t = trie({1, 1 - half}, key_set({1})); must(t.nodes.size() == 2 && t.nodes[1].ends == 2, "one element, one node"));
        BAD("a trie with a refused step", trie({1, 2, 11}, key_set({1, 2, -1, -4})));
        BAD("a trie with a step too large", trie({1, half}, pow2));
        GOOD("levels and positions", const RotTrie t = trie({3, 5, 7, 9, 11, 13}, pow2); for (size_t i = 0; i < t.nodes.size(); ++i) {
            const RotNode &nd = t.nodes[i];
            must(t.levels.at((size_t)nd.level).at((size_t)nd.pos) == (int)i, "levels and positions name each other");
            must(i == 0 || t.nodes[(size_t)nd.parent].level + 1 == nd.level, "a node lies one level below its parent");
        });
    }
    { // the 127 steps j * 128 of the BFV matrix product at N = 32768 under the power-of-two keys: 127 nodes
        const size_t N = 32768;
        std::unique_ptr<Params> pp(Params::create(kSchemeCKKS, N, {50, 50}, 0, false));
        std::set<uint32_t> pow2;
        for (int k = 0; ((size_t)1 << k) < N / 2; ++k) { pow2.insert(pp->galois_elt_from_step(1 << k)); pow2.insert(pp->galois_elt_from_step(-(1 << k))); }
        std::vector<int> steps;
        for (int j = 1; j < 128; ++j) steps.push_back(j * 128);
        GOOD("bfv_matmul", const RotTrie t = rotation_trie(*pp, steps.data(), (u64)steps.size(), [&](uint32_t e) { return pow2.count(e) != 0; });
             must(t.nodes.size() == 128, "127 key switches"));
    }
    if (failures) return 1;
    std::printf("rotation_plan ok\n");
    return 0;
}
