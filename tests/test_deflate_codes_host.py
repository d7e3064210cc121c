"""The serial Huffman code construction of the DEFLATE compressor (huff_lengths / huff_codes, snappy_amd/csrc/deflate_core.h:
what the CPU model runs and what the kernel's wave routines must equal) at its limits, against the independent reference
of tests/deflate_code_tables.py -- a heapq Huffman that follows the documented rules, exact rational Kraft sums, RFC 1951's
canonical codes.  The length limiter (15 bits for the literal/length and distance codes, 7 for the code length code)
practically never runs on whole inputs; here every alphabet gets tables built to need one tree, two, and three or more,
and the harness's count shows that they did.  The same tables go through the kernel in tests/test_gpu_deflate_edges.py."""
import collections

import numpy as np
import pytest

import deflate_code_tables as T
from test_f3_host import f3  # noqa: F401  (the host harness, built once per module)


def serial_tables(L, n, max_bits, tabs):
    """-> (lens, codes, rounds, depth0) of huff_lengths / huff_codes over tabs, through the harness."""
    freq = np.ascontiguousarray(np.stack([t for _, _, t in tabs]), dtype=np.uint32)
    nt = len(tabs)
    lens, codes = np.full((nt, n), 0xee, dtype=np.uint8), np.full((nt, n), 0xeeeeeeee, dtype=np.uint32)
    rounds, depth0 = np.zeros(nt, dtype=np.uint32), np.zeros(nt, dtype=np.uint32)
    assert L.f3_huff_tables(freq.ctypes.data, nt, n, max_bits, lens.ctypes.data, codes.ctypes.data, rounds.ctypes.data, depth0.ctypes.data) == 0
    return lens, codes, rounds, depth0


def in_group(group, rounds):
    return group is None or (rounds >= 3 if group == "3+" else rounds == int(group))


@pytest.mark.parametrize("n,max_bits", T.ALPHABETS)
def test_serial_codes_are_complete_canonical_and_limited(f3, n, max_bits):  # noqa: F811
    """Every table of the generator (seed: deflate_code_tables.SEED), none skipped: lengths within max_bits, a length for
    exactly the used symbols, Kraft sum 1 with two or more of them, length 1 for a lone one, canonical bit-reversed codes,
    the optimal cost wherever the unlimited tree fits -- and the lengths and the number of trees built equal what the
    documented rules give."""
    tabs = T.tables(n, max_bits)
    lens, codes, rounds, depth0 = serial_tables(f3, n, max_bits, tabs)
    for i, (name, _, freq) in enumerate(tabs):
        T.check_table(name, freq, max_bits, lens[i], codes[i], rounds[i], depth0[i])


@pytest.mark.parametrize("n,max_bits", T.ALPHABETS)
def test_every_table_needs_the_trees_it_is_meant_to(f3, n, max_bits):  # noqa: F811
    """The generator only aims; the harness's count shows that each group got there: one tree, two, three or more -- and
    that the ladders of every order and placement, the clamped weights and the raised 1 are among those that were rebuilt."""
    tabs = T.tables(n, max_bits)
    _, _, rounds, depth0 = serial_tables(f3, n, max_bits, tabs)
    seen = collections.Counter()
    for i, (name, group, _) in enumerate(tabs):
        assert in_group(group, int(rounds[i])), (name, group, int(rounds[i]), int(depth0[i]))
        assert (rounds[i] > 1) == (depth0[i] > max_bits), name  # rebuilt exactly when the first tree is too deep
        seen[group] += 1
    assert seen["1"] >= 20 and seen["2"] >= 18 and seen["3+"] >= 18, seen
    rebuilt = [name for i, (name, _, _) in enumerate(tabs) if rounds[i] >= 2]
    for what in ("fib", "pow2", " asc ", " desc ", " shuffled ", " at 0", "raised again", "zipf"):
        assert any(what in name for name in rebuilt), what
    if n == 286:  # the fifth slot of a lane, and across each slot's edge
        for at in (" at 256", " at 5", " at 11", " at 24"):
            assert any(at in name and ("fib" in name or "pow2" in name) for name in rebuilt), at
    # a weight that one halving takes to 0 and the rule raises to 1, in a table that was rebuilt
    assert any(rounds[i] >= 2 and (t == 1).any() for i, (_, _, t) in enumerate(tabs))
    # weights beyond 16 bits in a table that was rebuilt, and in one that was not
    assert any(rounds[i] >= 2 and (t > 0xffff).any() for i, (_, _, t) in enumerate(tabs))
    assert any(rounds[i] == 1 and (t > 0xffff).any() for i, (_, _, t) in enumerate(tabs))


def test_reference_is_not_the_routine_in_disguise():
    """The reference against facts that need no code: known optimal lengths, and a ladder's depth."""
    assert T.ref_lengths([5, 9, 12, 13, 16, 45], 15) == ([4, 4, 3, 3, 3, 1], 1)      # the textbook example
    assert sorted(T.ref_lengths([1, 1, 2, 3, 5, 8], 15)[0]) == [1, 2, 3, 4, 5, 5]
    assert T.ref_lengths(T.fib(17), 15)[1] == 2 and max(T.huffman_depths(T.fib(17))) == 16
    assert T.ref_codes([2, 1, 3, 3]) == [(0b01 << 8) | 2, (0 << 8) | 1, (0b011 << 8) | 3, (0b111 << 8) | 3]  # RFC 1951 3.2.2, reversed
    assert T.ref_lengths([1, 1, 2], 15)[0] == [2, 2, 1]  # 1 + 1 ties with the leaf of 2: the leaf goes first, either way the same depths


def test_harness_refuses_what_never_ends(f3):  # noqa: F811
    """More symbols than 2^max_bits can never fit: the harness (like snaphash_deflate_codes_device) refuses to start."""
    z = np.zeros(320, dtype=np.uint32)
    out = np.zeros(320, dtype=np.uint32)
    for n, mb in ((0, 15), (321, 15), (19, 4), (19, 0), (30, 16)):
        assert f3.f3_huff_tables(z.ctypes.data, 1, n, mb, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data) == -1
