"""The BFV selection tree (he355_bfv_select) restated with Python integers, twice over and independently of the library:

* the recursion of include/he355.h: the level table c_0 = count, c_(j+1) = ceil(c_j / 2), the pairs per level, the pass-through rule, and the
  leaf a bit vector selects -- by folding index lists level by level (`selected_leaf`) and by walking down from the root (`walk_leaf`);
* the noiseless CMUX on a small negacyclic ring Z_q[X] / (X^n + 1): node' = even + b (odd - even) with b the selector's bit as a constant
  polynomial, folded over polynomial leaves (`fold_polys`), which must return the selected leaf itself.
Used by tests/test_bfv_select_ref_cpu.py and tests/test_gpu_bfv_select.py."""


def depth(count):
    m = 0
    while (1 << m) < count:
        m += 1
    return m


def level_table(count):
    """[c_0, .., c_m]"""
    c = [count]
    while c[-1] > 1:
        c.append((c[-1] + 1) // 2)
    return c


def pairs_per_level(count):
    return [c // 2 for c in level_table(count)[:-1]]


def selected_leaf(count, bits):
    """fold the leaves' indices: bits[j] is consumed at level j, a node without a partner passes through whatever the bit says"""
    nodes = list(range(count))
    for j in range(depth(count)):
        nxt = []
        for p in range((len(nodes) + 1) // 2):
            if 2 * p + 1 < len(nodes):
                nxt.append(nodes[2 * p + 1] if bits[j] else nodes[2 * p])
            else:
                nxt.append(nodes[2 * p])
        nodes = nxt
    assert len(nodes) == 1
    return nodes[0]


def walk_leaf(count, bits):
    """the same leaf from the root down: node p of level j + 1 has the children 2p and 2p + 1 of level j, the second only if it exists"""
    c = level_table(count)
    p = 0
    for j in range(len(c) - 2, -1, -1):
        p = 2 * p + 1 if bits[j] and 2 * p + 1 < c[j] else 2 * p
    return p


def negacyclic_mul(a, b, q):
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            k = i + j
            if k < n:
                out[k] = (out[k] + x * y) % q
            else:
                out[k - n] = (out[k - n] - x * y) % q
    return out


def fold_polys(leaves, bits, q):
    """the noiseless CMUX tree over polynomial leaves (lists of n residues): even + bit (odd - even) in Z_q[X] / (X^n + 1)"""
    n = len(leaves[0])
    nodes = [list(x) for x in leaves]
    j = 0
    while len(nodes) > 1:
        b = [bits[j] % q] + [0] * (n - 1)
        nxt = []
        for p in range((len(nodes) + 1) // 2):
            if 2 * p + 1 < len(nodes):
                diff = [(o - e) % q for o, e in zip(nodes[2 * p + 1], nodes[2 * p])]
                nxt.append([(e + d) % q for e, d in zip(nodes[2 * p], negacyclic_mul(b, diff, q))])
            else:
                nxt.append(nodes[2 * p])
        nodes = nxt
        j += 1
    return nodes[0]
