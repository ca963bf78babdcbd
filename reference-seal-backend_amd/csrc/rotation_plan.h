// rotation_plan.h -- which Galois key switches a rotation step takes, and the trie that rotations of one ciphertext share: the host rule
// behind he355_rotate, he355_rotate_add, he355_rotate_sum and he355_rotate_each, spelt once.  Which Galois keys are installed is the device
// context's to know; it is asked through `has_key`, a predicate over Galois elements, and every refusal is made here, before the caller's
// first launch.  Host-only on purpose (he_params.h alone, no HIP header), in the style of hoist_args.h: tests/csim returns the plans to
// tests/test_rotation_plan_cpu.py, and tests/rotation_plan_main.cpp walks their edges under the sanitizers.
#pragma once
#include <algorithm>
#include <stdexcept>
#include <vector>

#include "he_params.h"

namespace he355 {

// Evaluator::rotate_internal: a step whose Galois element has a key of its own is one term; any other step takes its NAF terms, least
// significant first, a term of N / 2 being no rotation.  Step 0: no term.  Refused: |step| >= N / 2 ("step count too large"); a one-term
// NAF without its key, or a missing key of ANY term ("Galois key not present") -- a plan that comes back can be launched to its end.
template <class HasKey> std::vector<int> rotation_terms(const Params &p, int step, HasKey &&has_key)
{
    std::vector<int> terms;
    if (step == 0) return terms;
    const uint32_t elt = p.galois_elt_from_step(step);
    if (!elt) throw std::invalid_argument("step count too large");
    if (has_key(elt)) { terms.push_back(step); return terms; }
    const bool neg = step < 0;
    long v = neg ? -(long)step : step;
    int n_naf = 0;
    for (int i = 0; v; ++i) {
        const int zi = (v & 1) ? 2 - (int)(v & 3) : 0;
        v = (v - zi) >> 1;
        if (!zi) continue;
        ++n_naf;
        const long t = (neg ? -zi : zi) * (1L << i);
        if ((size_t)(t < 0 ? -t : t) != p.N / 2) terms.push_back((int)t);
    }
    if (n_naf == 1) throw std::invalid_argument("Galois key not present");
    for (int t : terms) {
        const uint32_t e = p.galois_elt_from_step(t);
        if (!e || !has_key(e)) throw std::invalid_argument("Galois key not present");
    }
    return terms;
}

// The term sequences of rotations that all start from ONE ciphertext form a trie: two steps whose sequences share a prefix share that
// prefix's intermediate ciphertext bit for bit, so each node is key-switched once, from its parent's ciphertext.  Node 0 is the input
// itself; `ends` counts the steps whose sequence ends at the node (node 0: the steps of 0); steps that differ by the row length are the
// same element, hence the same node.  levels[d] lists the nodes d terms deep in the order they were made, and a node's `pos` is its
// index there: the group index of a level-by-level walk.
struct RotNode {
    uint32_t elt;
    int parent;
    u64 ends;
    std::vector<int> kids;
    int level, pos;
};
struct RotTrie {
    std::vector<RotNode> nodes;
    std::vector<std::vector<int>> levels;
    size_t widest = 1; // nodes of the widest level
    size_t depth() const { return levels.size() - 1; }
};
template <class HasKey> RotTrie rotation_trie(const Params &p, const int *steps, u64 n_steps, HasKey &&has_key)
{
    RotTrie tr;
    tr.nodes.push_back(RotNode{0, -1, 0, {}, 0, 0});
    tr.levels.push_back({0});
    for (u64 j = 0; j < n_steps; ++j) {
        int at = 0;
        for (int t : rotation_terms(p, steps[j], has_key)) {
            const uint32_t te = p.galois_elt_from_step(t);
            int next = -1;
            for (int k : tr.nodes[(size_t)at].kids)
                if (tr.nodes[(size_t)k].elt == te) { next = k; break; }
            if (next < 0) {
                const size_t lv = (size_t)tr.nodes[(size_t)at].level + 1;
                if (lv == tr.levels.size()) tr.levels.emplace_back();
                next = (int)tr.nodes.size();
                tr.nodes.push_back(RotNode{te, at, 0, {}, (int)lv, (int)tr.levels[lv].size()});
                tr.nodes[(size_t)at].kids.push_back(next);
                tr.levels[lv].push_back(next);
                tr.widest = std::max(tr.widest, tr.levels[lv].size());
            }
            at = next;
        }
        ++tr.nodes[(size_t)at].ends;
    }
    return tr;
}

} // namespace he355
