"""The rotation plans of csrc/rotation_plan.h -- the terms of a rotation step (Evaluator::rotate_internal's rule: the step's own Galois key,
else its NAF terms least significant first, a term of N / 2 being no rotation) and the trie the rotations of one ciphertext share, the one
host rule behind he355_rotate, he355_rotate_add, he355_rotate_sum and he355_rotate_each -- held to tests/launch_plan.py's restatement
(`naf_terms`, `rotation_terms`, `rotation_trie_nodes`, `rotation_trie_levels`) through tests/csim's entry points.  The header takes its key set
as a predicate over Galois elements, the restatement as steps: the two meet through `launch_plan.galois_elt`.

* every step of N = 1024, the edges of N = 8192, under four kinds of key set: the power-of-two steps, ROTATE_KEY_STEPS, every step (each is
  one term), and a set that holds a step's own key and lacks one of its NAF terms;
* refusals, each with nothing written: |step| >= N / 2 ("step count too large"); a one-term NAF without its key, and a several-term step that
  lacks its first, a middle or its last term's key ("Galois key not present");
* tries: ROTATE_SUM_STEPS, the j 2^k family of the bfv_matmul shape (127 nodes for 313 terms), repeated steps, steps of 0, two steps that differ
  by the row length (one element, one node); per node its element, parent, ends, level and position.
And the header under the sanitizers: tests/rotation_plan_main.cpp, a stand-alone program, walks the same edges; compiled with
g++ -fsanitize=address,undefined, the runtimes linked statically, and run as a child process.
No GPU."""
import ctypes as C

import pytest

import csim_lib
import launch_plan as lp
import sanitized_program

TOO_LARGE, NO_KEY = -1, -2
SENTINEL = 0x5A5A5A5
CAP = 4096


@pytest.fixture(scope="module")
def sim():
    L = csim_lib.load()
    L.sim_params_create.restype = C.c_void_p
    L.sim_params_create.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_int), C.c_size_t, C.c_int, C.c_int]
    L.sim_params_destroy.argtypes = [C.c_void_p]
    L.sim_galois_elt.restype = C.c_uint32
    L.sim_galois_elt.argtypes = [C.c_void_p, C.c_int]
    i32p, u32p, u64p = C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.sim_rotation_terms.restype = C.c_long
    L.sim_rotation_terms.argtypes = [C.c_void_p, C.c_int, u32p, C.c_size_t, i32p, C.c_size_t]
    L.sim_rotation_trie.restype = C.c_long
    L.sim_rotation_trie.argtypes = [C.c_void_p, i32p, C.c_size_t, u32p, C.c_size_t, u32p, i32p, u64p, i32p, i32p, C.c_size_t]
    return L


@pytest.fixture(scope="module")
def rings(sim):
    """Params handles of the rings the cases use, made once"""
    bits = (C.c_int * 2)(50, 50)
    hs = {N: sim.sim_params_create(2, N, bits, 2, 0, 0) for N in (1024, 8192, 32768)}
    assert all(hs.values())
    yield hs
    for h in hs.values():
        sim.sim_params_destroy(h)


def elts_of(steps, N):
    return sorted({lp.galois_elt(s, N) for s in steps})


def pow2_steps(N):
    return [s for k in range((N // 2).bit_length() - 1) for s in (1 << k, -(1 << k))]  # +-2^k, 2^k < N / 2


def terms_of(sim, h, step, key_elts):
    """(return code or number of terms, the terms, whether the buffer behind them is untouched)"""
    keys = (C.c_uint32 * max(1, len(key_elts)))(*key_elts)
    buf = (C.c_int * 64)(*([SENTINEL] * 64))
    r = sim.sim_rotation_terms(h, step, keys, len(key_elts), buf, 64)
    k = max(r, 0)
    return r, list(buf[:k]), all(x == SENTINEL for x in buf[k:])


def expected_terms(step, N, key_elts):
    """the restatement's terms, or the refusal: launch_plan has no refusals of its own, the rule's are spelt here"""
    if step == 0:
        return []
    if abs(step) >= N // 2:
        return TOO_LARGE
    own = lp.galois_elt(step, N) in key_elts
    terms = lp.rotation_terms(step, N, (step,) if own else ())
    if own:
        return terms
    if len(lp.naf_terms(step, 1 << 40)) == 1:  # (a ring so large that no term is dropped: the NAF's own length)
        return NO_KEY
    return terms if all(lp.galois_elt(t, N) in key_elts for t in terms) else NO_KEY


def check_step(sim, h, N, step, key_elts):
    r, got, clean = terms_of(sim, h, step, key_elts)
    want = expected_terms(step, N, set(key_elts))
    assert clean, (N, step)
    if isinstance(want, int):
        assert r == want and not got, (N, step, r, want)
    else:
        assert r == len(want) and got == want, (N, step, got, want)
    return want


def test_galois_elt_restated(sim, rings):
    for N, h in rings.items():
        for s in (0, 1, -1, 3, -3, N // 4, -(N // 4), N // 2 - 1, -(N // 2 - 1)):
            assert sim.sim_galois_elt(h, s) == lp.galois_elt(s, N), (N, s)


def test_every_step_of_n1024_under_each_key_set(sim, rings):
    N, h = 1024, rings[1024]
    steps = range(-(N // 2 - 1), N // 2)
    every = elts_of([s for s in steps if s], N)
    outcomes = set()
    for keys in (elts_of(pow2_steps(N), N), elts_of(lp.ROTATE_KEY_STEPS, N), every):
        for s in steps:
            want = check_step(sim, h, N, s, keys)
            outcomes.add("refused" if isinstance(want, int) else min(len(want), 2))
        if keys is every:
            assert all(expected_terms(s, N, set(keys)) == [s] for s in steps if s)
    assert outcomes == {"refused", 0, 1, 2}  # every kind of answer was seen
    # a term of N / 2 is dropped: N / 2 - 3 = 1 - 4 + N / 2 is two rotations (N / 2 - 1 is the element of -1: its own key)
    assert check_step(sim, h, N, N // 2 - 3, elts_of(pow2_steps(N), N)) == [1, -4]
    assert check_step(sim, h, N, N // 2 - 1, elts_of(pow2_steps(N), N)) == [N // 2 - 1]


def test_edges_of_n8192(sim, rings):
    N, h = 8192, rings[8192]
    edges = (1, -1, N // 2 - 1, -(N // 2 - 1), N // 4, -(N // 4), 0)
    for keys in (elts_of(pow2_steps(N), N), elts_of(lp.ROTATE_KEY_STEPS, N), elts_of([s for s in edges if s], N)):
        for s in edges:
            check_step(sim, h, N, s, keys)
    assert check_step(sim, h, N, N // 2 - 3, elts_of(pow2_steps(N), N)) == [1, -4]
    assert check_step(sim, h, N, -(N // 2 - 3), elts_of(pow2_steps(N), N)) == [-1, 4]
    assert check_step(sim, h, N, 3, elts_of(lp.ROTATE_KEY_STEPS, N)) == [-1, 4]


@pytest.mark.parametrize("N", [1024, 8192])
def test_own_key_wins_over_missing_naf_terms(sim, rings, N):
    """a step with a key of its own is one term whether or not its NAF terms have keys"""
    h = rings[N]
    assert check_step(sim, h, N, 3, elts_of([3, -1], N)) == [3]       # lacks 4
    assert check_step(sim, h, N, 11, elts_of([11], N)) == [11]        # lacks -1, -4 and 16
    assert check_step(sim, h, N, 3 - N // 2, elts_of([3], N)) == [3 - N // 2]  # the same element as 3: its key is this step's own


@pytest.mark.parametrize("N", [1024, 8192])
def test_refusals(sim, rings, N):
    h = rings[N]
    keys = elts_of(pow2_steps(N), N)
    for s in (N // 2, -(N // 2), N // 2 + 1, N, 2 ** 31 - 1, -2 ** 31):
        assert check_step(sim, h, N, s, keys) == TOO_LARGE
    assert check_step(sim, h, N, 8, elts_of(lp.ROTATE_KEY_STEPS, N)) == NO_KEY  # a one-term NAF without its key
    assert check_step(sim, h, N, -8, elts_of(lp.ROTATE_KEY_STEPS, N)) == NO_KEY
    assert check_step(sim, h, N, 5, []) == NO_KEY
    assert lp.naf_terms(11, N) == [-1, -4, 16]
    assert check_step(sim, h, N, 11, elts_of([-1, -4, 16], N)) == [-1, -4, 16]
    for missing in (-1, -4, 16):  # its first, a middle and its last term: refused whole, nothing written
        assert check_step(sim, h, N, 11, elts_of([t for t in (-1, -4, 16) if t != missing], N)) == NO_KEY
    # a trie is refused as a whole when one step of it is
    assert trie_of(sim, h, [1, 2, 11], elts_of([1, 2, -1, -4], N)) == NO_KEY
    assert trie_of(sim, h, [1, N // 2], keys) == TOO_LARGE


def trie_of(sim, h, steps, key_elts):
    """the return code, or the nodes as [(element, parent, ends, level, position)]"""
    keys = (C.c_uint32 * max(1, len(key_elts)))(*key_elts)
    st = (C.c_int * max(1, len(steps)))(*steps)
    elt, parent, ends = (C.c_uint32 * CAP)(), (C.c_int * CAP)(*([SENTINEL] * CAP)), (C.c_uint64 * CAP)()
    level, pos = (C.c_int * CAP)(), (C.c_int * CAP)()
    r = sim.sim_rotation_trie(h, st, len(steps), keys, len(key_elts), elt, parent, ends, level, pos, CAP)
    if r < 0:
        assert all(x == SENTINEL for x in parent)
        return r
    return [(elt[i], parent[i], ends[i], level[i], pos[i]) for i in range(r)]


def check_trie(sim, h, N, steps, key_steps):
    key_elts = elts_of(key_steps, N)
    nodes = trie_of(sim, h, steps, key_elts)
    assert not isinstance(nodes, int), nodes
    # the restatement keys its prefixes by steps; a step counts as keyed when its ELEMENT has a key, and prefixes meet through their elements
    keyed = [s for s in steps if s and lp.galois_elt(s, N) in key_elts]
    restated = lp.rotation_trie_nodes(steps, N, keyed)
    want = {}
    for prefix, (ends, kids) in restated.items():
        e = want.setdefault(tuple(lp.galois_elt(t, N) for t in prefix), [0, False])
        e[0] += ends
        e[1] = e[1] or kids
    # node 0 is the input itself: no element, no parent, the steps of 0 end there
    assert nodes[0] == (0, -1, sum(1 for s in steps if s == 0), 0, 0)
    got, paths, seen_at_level = {}, {0: ()}, {0: 1}
    has_kids = {p for (_, p, _, _, _) in nodes[1:]}
    for i, (elt, parent, ends, level, pos) in enumerate(nodes[1:], start=1):
        assert 0 <= parent < i and level == nodes[parent][3] + 1 and elt % 2 == 1
        assert pos == seen_at_level.get(level, 0)  # the position is the node's rank among the nodes of its level, in node order
        seen_at_level[level] = pos + 1
        paths[i] = paths[parent] + (elt,)
        assert paths[i] not in got  # one node per element path
        got[paths[i]] = [ends, i in has_kids]
    assert got == want
    widths = [seen_at_level[d] for d in sorted(seen_at_level) if d]
    assert widths == [sum(1 for path in want if len(path) == d) for d in range(1, len(widths) + 1)]
    if len(want) == len(restated):  # (no two term prefixes of one element path: the restated widths count the same nodes)
        assert widths == lp.rotation_trie_levels(steps, N, keyed)
    return nodes, widths


def test_trie_of_the_rotate_sum_cases(sim, rings):
    N, h = 8192, rings[8192]
    nodes, widths = check_trie(sim, h, N, lp.ROTATE_SUM_STEPS, lp.ROTATE_KEY_STEPS)
    assert widths == [3, 1] and len(nodes) == 5  # 1, 2, -1 and, under -1, 4
    e = lambda s: lp.galois_elt(s, N)
    assert nodes == [(0, -1, 0, 0, 0), (e(1), 0, 1, 1, 0), (e(2), 0, 1, 1, 1), (e(-1), 0, 0, 1, 2), (e(4), 3, 1, 2, 0)]


def test_trie_of_the_bfv_matmul_shape(sim, rings):
    """steps j 2^k, j = 1 .. 127, under the +-2^k key set: every prefix of a NAF sequence is the NAF sequence of a smaller j -- 127 key
    switches for the 313 terms of the reference's loop"""
    N, h = 32768, rings[32768]
    spacers = (N // 2) // 128
    steps = [j * spacers for j in range(1, 128)]
    nodes, widths = check_trie(sim, h, N, steps, pow2_steps(N))
    assert len(nodes) - 1 == 127 and widths == [13, 50, 56, 8]
    assert sum(len(lp.rotation_terms(s, N, pow2_steps(N))) for s in steps) == 313
    assert all(ends == 1 for (_, _, ends, _, _) in nodes[1:])


def test_trie_of_repeats_zeros_and_one_element_twice(sim, rings):
    N, h = 1024, rings[1024]
    nodes, widths = check_trie(sim, h, N, [3, 3, 0, 1, 0, 3], lp.ROTATE_KEY_STEPS)
    assert nodes[0][2] == 2 and widths == [2, 1]  # two steps of 0; -1 and 1, then 4 under -1 with three ends
    assert [n for n in nodes if n[2] == 3] == [(lp.galois_elt(4, N), 1, 3, 2, 0)]
    nodes, _ = check_trie(sim, h, N, [], lp.ROTATE_KEY_STEPS)
    assert nodes == [(0, -1, 0, 0, 0)]
    nodes, _ = check_trie(sim, h, N, [0, 0], [])
    assert nodes == [(0, -1, 2, 0, 0)]
    # 1 and 1 - N / 2 are the same rotation, the same key: one node where two steps end; so below a shared first term
    assert lp.galois_elt(1, N) == lp.galois_elt(1 - N // 2, N)
    nodes, widths = check_trie(sim, h, N, [1, 1 - N // 2], [1])
    assert nodes == [(0, -1, 0, 0, 0), (lp.galois_elt(1, N), 0, 2, 1, 0)] and widths == [1]
    nodes, widths = check_trie(sim, h, N, [3, 5, 4 - N // 2], [1, -1, 4])
    assert widths == [3, 2]  # -1, 1 and 4's element at the first level (the last step's own key); 4 under -1 and under 1


def test_the_header_under_the_sanitizers(tmp_path):
    sanitized_program.run(tmp_path, "rotation_plan_main.cpp", "rotation_plan ok")
