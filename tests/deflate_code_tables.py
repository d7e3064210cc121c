"""Frequency tables that drive the DEFLATE compressor's Huffman code construction to its limits, and an independent
reference for what it must leave.  Shared by tests/test_deflate_codes_host.py (the serial routines of deflate_core.h)
and tests/test_gpu_deflate_edges.py (huff_lengths_wave / huff_codes_wave through snaphash_deflate_codes_device).

A tree deeper than max_bits makes both routines halve the weights (never to 0, at most 0xffff) and build again.  Whole
inputs practically never get there -- the price parse flattens the histogram -- so the tables are handed to the routines
directly.  Every table names the number of trees it is MEANT to need ("1", "2", "3+", or None where it is left open);
the tests hold the harness's count against that.

The reference is a heapq Huffman that follows the documented rules only (deflate_core.h: stable order by weight then
symbol index, a tie between a leaf and an internal node goes to the leaf, internal nodes first made first taken), exact
rational Kraft sums, and RFC 1951's canonical code assignment."""
import heapq
from fractions import Fraction

import numpy as np

SEED = 1951                                   # of every random table below
ALPHABETS = ((286, 15), (30, 15), (19, 7))    # (symbols, max_bits): literal/length, distance, code length code
N_RANDOM = 300                                # Zipf tables per alphabet


def fib(k):
    out, a, b = [], 1, 1
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return out


def pow2(k):
    return [1 << i for i in range(k)]


def expected_rounds(kind, k, max_bits):
    """Trees a k-symbol ladder is meant to need.  Its first tree is k - 1 deep.  Halving a 2^i ladder once leaves it as
    deep (its two lightest weigh 1 and 1 then, and their sum ties with the leaf of 2, which goes first); from the second
    halving on it loses a level a round: three trees at the least.  A halving takes up to three levels off a Fibonacci
    ladder (1 1 1 1 2 4 6 10 ... for 1 1 2 3 5 8 13 21 ...): one to three levels too many are gone after one."""
    over = (k - 1) - max_bits  # levels too many
    if over <= 0:
        return "1"
    if kind == "pow2":
        return "3+"
    return "2" if over <= 3 else "3+"


def _place(n, start, weights, order, rng):
    t = np.zeros(n, dtype=np.uint64)
    w = list(weights)
    if order == "desc":
        w = w[::-1]
    elif order == "shuffled":
        w = [w[i] for i in rng.permutation(len(w))]
    t[start:start + len(w)] = w
    return t


def tables(n, max_bits):
    """-> list of (name, meant rounds or None, numpy uint32[n])."""
    rng = np.random.default_rng(SEED + 1000 * n + max_bits)
    out = []

    def add(name, group, t):
        t = np.asarray(t, dtype=np.uint64)
        assert t.shape == (n,) and int(t.max(initial=0)) <= 0xffffffff, name
        out.append(("%d/%d %s" % (n, max_bits, name), group, t.astype(np.uint32)))

    # ---- ladders over the smallest symbol counts that overflow the limit (and the last that fits) ----
    kmax = min(n, 30 if max_bits == 15 else 19)
    for k in range(max_bits + 1, kmax + 1):
        starts = {0, n - k}                                   # from the first symbol; up to the last
        for edge in (64, 128, 256):                           # straddling a lane's next slot
            if edge - k // 2 >= 0 and edge - k // 2 + k <= n:
                starts.add(edge - k // 2)
        if 256 + k <= n:
            starts.add(256)                                   # wholly in the fifth slot of a lane
        for kind, w in (("fib", fib(k)), ("pow2", pow2(k))):
            for order in ("asc", "desc", "shuffled"):
                for s in sorted(starts):
                    add("%s k=%d %s at %d" % (kind, k, order, s), expected_rounds(kind, k, max_bits), _place(n, s, w, order, rng))
    # ---- weights up to what a chunk can hold (65536 tokens) and beyond the 16 bits a weight keeps ----
    k = min(n, max_bits + 4)
    add("one symbol has the chunk, the rest 1 each", "1", [65536 - (n - 1)] + [1] * (n - 1))
    add("65535 | 1", "1", [65535, 1] + [0] * (n - 2))
    add("65536 | 1: clamped", "1", [65536, 1] + [0] * (n - 2))
    add("all 0xffffffff: every weight clamps alike", "1", [0xffffffff] * n)
    add("0xffff, 0x10000, 0x12345, 0xffffffff weigh the same", "1", ([0xffff, 0x10000, 0x12345, 0xffffffff] * n)[:n])
    add("fib * 65536: clamped flat", "1", _place(n, 0, [f << 16 for f in fib(k) if f << 16 <= 0xffffffff], "asc", rng))
    add("fib * 16 above a lone 1: the 1 is halved to 0 and raised again", "3+", _place(n, 0, [1] + [16 * f for f in fib(k - 1)], "asc", rng))
    # (of 19 symbols all but three weigh 0xffff: flat)
    add("pow2 ladder to 2^31", "1" if n < 24 else "3+", _place(n, 0, [1 << (31 - i) for i in range(min(n, 32))], "asc", rng))
    add("fib ladder sums to a chunk", "3+", _place(n, n - min(n, 23), fib(min(n, 23)), "shuffled", rng))
    # ---- flat and nearly empty ----
    for v in (1, 7, 0xffff, 0x10000):
        add("all %d" % v, "1", [v] * n)
    add("nothing used", "1", [0] * n)
    for pos in sorted({0, 1, n // 2, n - 1, min(n - 1, 63), min(n - 1, 64), min(n - 1, 256)}):
        t = np.zeros(n, dtype=np.uint64)
        t[pos] = 5
        add("one symbol used: %d" % pos, "1", t)
    for a, b in ((0, 1), (0, n - 1), (n - 2, n - 1), (min(63, n - 2), min(64, n - 1))):
        t = np.zeros(n, dtype=np.uint64)
        t[a], t[b] = 3, 70000
        add("two symbols used: %d %d" % (a, b), "1", t)
    for tri in ((0, 1, 2), (0, n // 2, n - 1), (n - 3, n - 2, n - 1)):
        for w in ((1, 1, 1), (1, 1, 2), (5, 3, 1)):
            t = np.zeros(n, dtype=np.uint64)
            for p, v in zip(tri, w):
                t[p] = v
            add("three symbols used: %s weights %s" % (tri, w), "1", t)
    add("every symbol used: 1..n", "1", np.arange(1, n + 1))
    add("every symbol used: n..1", "1", np.arange(n, 0, -1))
    add("every symbol used: random", "1", rng.integers(1, 1000, size=n))
    # ---- many ties between a leaf and an internal node ("the leaf first") ----
    add("ties: 1 1 2 2 4 4 ...", None, ([1 << (i // 2) for i in range(min(n, 32))] + [0] * n)[:n])
    add("ties: 1 1 2 4 8 ... (every sum meets a leaf)", None, ([1] + pow2(min(n, 24) - 1) + [0] * n)[:n])
    add("ties: 3 3 6 12 24 ... descending", None, (([3] + [3 << i for i in range(min(n, 14) - 1)])[::-1] + [0] * n)[:n])
    add("ties: 1 1 1 1 2 2 4 4 4 8 ...", None, ([1, 1, 1, 1, 2, 2, 4, 4, 4, 8, 8, 16, 16, 16, 32, 64, 64, 128] + [0] * n)[:n])
    add("ties: all 2 but two 1s", "1", [1, 1] + [2] * (n - 2))
    for i in range(8):
        add("ties: weights from {1,2,3,4} #%d" % i, "1", rng.integers(1, 5, size=n))
        t = rng.choice(np.array([1, 2, 4, 8, 16, 32], dtype=np.uint64), size=n)
        t[rng.random(n) < 0.3] = 0
        add("ties: powers of two with gaps #%d" % i, None, t)
    # ---- seeded random tables, Zipf weights ----
    for i in range(N_RANDOM):
        a = (1.1, 1.3, 1.6, 2.0, 3.0)[i % 5]
        t = rng.zipf(a, size=n).astype(np.float64)
        t = np.minimum(t * float(rng.choice([1, 1, 3, 64, 1000, 70000])), 0xffffffff).astype(np.uint64)
        used = rng.random(n) < rng.choice([0.1, 0.4, 0.8, 1.0])
        t[~used] = 0
        add("zipf %.1f #%d" % (a, i), None, t)
    return out


def all_tables():
    return {(n, mb): tables(n, mb) for n, mb in ALPHABETS}


# ---- the reference --------------------------------------------------------------------------------------------------

def weights_of_round(freq, r):
    return [0 if f == 0 else min(max(int(f) >> r, 1), 0xffff) for f in freq]


def huffman_depths(w):
    """Depths of the tree the documented rules give for weights w (0 = unused); two or more used symbols."""
    heap = [(x, 0, i) for i, x in enumerate(w) if x]
    heapq.heapify(heap)
    kids, seq = [], 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        kids.append((a, b))
        heapq.heappush(heap, (a[0] + b[0], 1, seq))
        seq += 1
    depth = [0] * len(w)
    todo = [(heap[0], 0)]
    while todo:
        (_, internal, i), d = todo.pop()
        if internal:
            todo += [(kids[i][0], d + 1), (kids[i][1], d + 1)]
        else:
            depth[i] = d
    return depth


def optimal_cost(w):
    """Weighted length of ANY Huffman code for w: the sum of the merged weights (plain heapq, no rule for ties)."""
    heap = [x for x in w if x]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        s = heapq.heappop(heap) + heapq.heappop(heap)
        cost += s
        heapq.heappush(heap, s)
    return cost


def ref_lengths(freq, max_bits):
    """-> (lengths, trees built)."""
    n = len(freq)
    for r in range(33):
        w = weights_of_round(freq, r)
        used = [i for i in range(n) if w[i]]
        if len(used) <= 1:
            return [1 if w[i] else 0 for i in range(n)], r + 1
        d = huffman_depths(w)
        if max(d) <= max_bits:
            return d, r + 1
    raise AssertionError("no tree of %d symbols fits %d bits" % (n, max_bits))


def ref_codes(lens):
    """RFC 1951 sec. 3.2.2 -> code << 8 | length, the code bit-reversed (Huffman codes go out MSB first into an LSB-first stream)."""
    top = max(max(lens), 1)
    count = [0] * (top + 2)
    for b in lens:
        count[b] += 1
    count[0] = 0
    nxt, code = [0] * (top + 2), 0
    for b in range(1, top + 1):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for b in lens:
        if not b:
            out.append(0)
            continue
        c = nxt[b]
        nxt[b] += 1
        assert c < (1 << b)
        out.append((int(format(c, "0%db" % b)[::-1], 2) << 8) | b)
    return out


def check_table(name, freq, max_bits, lens, codes, rounds, depth0=None):
    """Everything a code must be, whoever built it: lens / codes / rounds as the routine under test left them."""
    freq = [int(f) for f in freq]
    lens = [int(x) for x in lens]
    used = [i for i, f in enumerate(freq) if f]
    assert max(lens, default=0) <= max_bits, name
    assert all((lens[i] >= 1) == (freq[i] != 0) for i in range(len(freq))), name
    if len(used) == 1:
        assert lens[used[0]] == 1, name
    if len(used) >= 2:
        assert sum(Fraction(1, 1 << b) for b in lens if b) == 1, name   # a complete prefix code
    assert [int(c) for c in codes] == ref_codes(lens), name
    want, want_rounds = ref_lengths(freq, max_bits)
    assert int(rounds) == want_rounds, (name, int(rounds), want_rounds)
    assert lens == want, name
    if len(used) >= 2:
        d0 = max(huffman_depths(weights_of_round(freq, 0)))
        if depth0 is not None:
            assert int(depth0) == d0, name
        if d0 <= max_bits:  # the unlimited tree fits: the code is optimal
            w = weights_of_round(freq, 0)
            assert sum(w[i] * lens[i] for i in used) == optimal_cost(w), name
