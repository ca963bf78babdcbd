"""tests/bfv_select_ref.py held to itself, exhaustively for count <= 9 (every bit vector of every count):

* the level table ends in 1 after ceil(log2 count) levels, halves with the ceiling, and its pairs plus pass-through nodes account for every node;
* folding index lists and walking down from the root name the same leaf; where sum b_j 2^j < count that leaf is the index itself, and where it
  is not the leaf is still below count (the pass-through rule decides: count = 5, bits (1, 0, 1) give leaf 4);
* every leaf is reachable;
* the noiseless CMUX over polynomial leaves on negacyclic rings of 4 and 8 coefficients, under a 17-bit, a 40-bit and a 45-bit modulus,
  returns exactly the selected leaf's polynomial.
No GPU."""
import itertools
import random

import pytest

import bfv_select_ref as ref

COUNTS = range(1, 10)


def test_level_tables():
    assert ref.level_table(1) == [1] and ref.level_table(2) == [2, 1] and ref.level_table(5) == [5, 3, 2, 1] and ref.level_table(9) == [9, 5, 3, 2, 1]
    for count in list(COUNTS) + [31, 32, 33, 1023, 1025, 1 << 20]:
        c = ref.level_table(count)
        m = ref.depth(count)
        assert len(c) == m + 1 and c[0] == count and c[-1] == 1 and (1 << m) >= count and (m == 0 or (1 << (m - 1)) < count)
        pairs = ref.pairs_per_level(count)
        for j in range(m):
            assert c[j + 1] == -(-c[j] // 2) and pairs[j] + (c[j] & 1) == c[j + 1] and 2 * pairs[j] + (c[j] & 1) == c[j]
        assert c[1:2] == ([-(-count // 2)] if m else []) and c[2:3] == ([-(-count // 4)] if m >= 2 else [])


@pytest.mark.parametrize("count", COUNTS)
def test_which_leaf_every_bit_vector(count):
    m = ref.depth(count)
    seen = set()
    for bits in itertools.product((0, 1), repeat=m):
        leaf = ref.selected_leaf(count, bits)
        assert leaf == ref.walk_leaf(count, bits) and 0 <= leaf < count
        idx = sum(b << j for j, b in enumerate(bits))
        if idx < count:
            assert leaf == idx
        seen.add(leaf)
    assert seen == set(range(count))
    if count == 5:
        assert ref.selected_leaf(5, (1, 0, 1)) == 4 and ref.selected_leaf(5, (1, 1, 1)) == 4 and ref.selected_leaf(5, (0, 1, 1)) == 4


@pytest.mark.parametrize("n,q", [(4, 65537), (8, 1099511480321), (4, 0x1fffffff9001)])  # the last: prime 0 of (1024, {45, 55, 50})
def test_noiseless_cmux_returns_the_selected_leaf(n, q):
    rng = random.Random(7 * n)
    for count in COUNTS:
        leaves = [[rng.randrange(q) for _ in range(n)] for _ in range(count)]
        leaves[0][0], leaves[-1][-1] = q - 1, 0
        for bits in itertools.product((0, 1), repeat=ref.depth(count)):
            assert ref.fold_polys(leaves, bits, q) == leaves[ref.selected_leaf(count, bits)], (count, bits)
