// behz_lists.h -- the operand-list geometry of the BEHZ multiply (DeviceContext::bfv_multiply3): which distinct operands a batch of n
// results reads, whether extending each of them once can replace the per-pair path, and the words of scratch either path takes.  The
// overlap refusal, the fit of the scratch to the device and the launches stay with the device context.  Host-only on purpose
// (device_types.h alone, no HIP header), in the style of rotation_plan.h: tests/csim returns the geometry to
// tests/test_bfv_multiply_plan_cpu.py and tests/test_behz_sim_cpu.py, and tests/shape_rules_main.cpp walks its edges under the sanitizers.
#pragma once
#include <algorithm>
#include <cstddef>

#include "device_types.h"

namespace he355 {

struct BehzLists {
    u64 G, I, J, na, n_cts; // groups of the batch; a's and b's per group; all a's; all distinct operands (BehzSrc: I, J, na)
    bool may_list;          // the operand lists apply: at least two times fewer extensions than the 2 n of the per-pair path
    size_t e_words;         // lists: the extended and transformed operand set, words
    size_t per_res;         // both paths: the three products of one result under q and Bsk, words
    size_t per_op;          // per-pair path: one result with its four extended polynomials, words
    size_t a_cts, b_cts;    // ciphertexts of `a` / `b` up to the last one read (the overlap check's spans)
};
// L data primes, S = nB + 1 residues of the auxiliary base, ring of N coefficients
inline BehzLists behz_lists(const Indexer3 &ix, u64 n, int L, size_t S, size_t N)
{
    BehzLists g;
    // Distinct operands: result r = (g, i, j) reads a(g, i) and b(g, j).  Where every operand serves several results (outer products,
    // the terms of a matrix product) each is extended to Bsk and transformed ONCE (steps (1)-(3) per operand instead of per result:
    // SEAL's multiply recomputes them for every pair, the values are the same), and a result costs its dyadic tensor, three inverse
    // transforms and steps (6)-(8).
    const u64 gsz = std::min<u64>(ix.gs, n);
    g.G = ix.gs >= n ? 1 : (n + ix.gs - 1) / ix.gs;
    g.I = (gsz + ix.b1 - 1) / ix.b1; g.J = std::min<u64>(ix.b1, gsz); g.na = g.G * g.I;
    g.n_cts = g.na + g.G * g.J;
    g.e_words = (size_t)g.n_cts * 2 * (L + S) * N; g.per_res = (3 * L + 3 * S) * N;
    g.per_op = (4 * L + 4 * S) * N + g.per_res;
    g.a_cts = (size_t)(ix.a_base + (g.G - 1) * ix.a_sg + (g.I - 1) * ix.a_si + 1); g.b_cts = (size_t)(ix.b_base + (g.G - 1) * ix.b_sg + (g.J - 1) * ix.b_sj + 1);
    g.may_list = (g.G == 1 || (n % ix.gs == 0 && ix.gs % ix.b1 == 0)) && g.n_cts <= n;
    return g;
}

} // namespace he355
