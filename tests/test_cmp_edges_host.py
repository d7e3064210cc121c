"""The cases of tests/cmp_edge_cases.py on the CPU: the closed-form verdicts of every group are the ones a plain byte
compare (ranges_equal_ref) gives over the built bytes, every range and the 16-byte piece that holds its last byte lie
inside its buffer, the slack behind a range differs between the two sides, and every group has the flips it claims --
so that a wrong verdict in tests/test_gpu_cmp_edges.py points at ranges_equal_kernel, launch_compare_ranges or
files_equal_impl, not at the inputs."""
import numpy as np
import pytest

import cmp_edge_cases as E


def check(case, lay=None, mixed=True):
    lay = lay or E.materialise(case)
    assert E.in_bounds(lay), case["name"]
    want = E.ranges_equal_ref(lay["a"], lay["off_a"], lay["b"], lay["off_b"], lay["lens"])
    assert np.array_equal(want, case["expected"]), (case["name"], E.report(case, want))
    if mixed:
        assert want.any() and not want.all(), case["name"]
    return lay, want


def unmasked_differs(lay, pick):
    """A compare of whole 16-byte pieces says "differ" for every picked pair whose length is no multiple of 16: the
    slack makes a missing tail mask visible."""
    pick = [i for i in pick if int(lay["lens"][i]) % 16]
    sub = lambda k: lay[k][pick]
    got = E.ranges_equal_ref(lay["a"], sub("off_a"), lay["b"], sub("off_b"), E.pad16(sub("lens").astype(np.int64)))
    return len(pick) > 0 and not got.any()


@pytest.mark.parametrize("n", E.A_LENGTHS)
def test_group_a_flips_every_piece(n):
    case = E.group_a_case(n)
    lay, want = check(case)
    npieces = (n + 15) // 16
    assert len(want) == npieces + 1 and not want[:-1].any() and want[-1] == 1
    assert np.array_equal(case["flip_pair"], np.arange(npieces))  # one flip each, the last pair has none
    assert np.array_equal(case["flip_pos"] // 16, np.arange(npieces)) and np.all(case["flip_pos"] < n)
    assert len(set(lay["off_a"].tolist())) == 1 and lay["off_a"][0] != 0 and len(set(lay["off_b"].tolist())) == len(want)
    if n % 16:
        assert unmasked_differs(lay, [npieces])  # the unflipped pair


def visited(nbytes, drop=None):
    """The pieces of one chunk that ranges_equal_kernel's two loops look at, restated lane by lane; drop="k3": the
    unrolled loop without its fourth piece, drop="handover": the stride-256 loop starting one step late."""
    npieces, nwhole = (nbytes + 15) >> 4, nbytes >> 4
    seen = np.zeros(npieces, dtype=bool)
    for lane in range(256):
        p = lane
        while p + 768 < nwhole:
            seen[[p + 256 * k for k in range(3 if drop == "k3" else 4)]] = True
            p += 1024
        p += 256 if drop == "handover" else 0
        while p < npieces:
            seen[p] = True
            p += 256
    return seen


def test_group_a_lengths_sit_on_the_loop_bounds():
    """Why these lengths: at each of them the restated loops see every piece, and among them are lengths at which a
    single lane takes a trip of the unrolled loop (nwhole = 769, 1793), all lanes do (1024, 2048), and none does."""
    for n in E.A_LENGTHS:
        assert visited(n).all(), n
    trips = {n: sum(1 for lane in range(256) if lane + 768 < n >> 4) for n in E.A_LENGTHS}
    assert {0, 1, 255, 256} <= set(trips.values())
    assert trips[16 * 768] == 0 and trips[16 * 769] == 1 and trips[16 * 1024] == 256 and trips[16 * 1792 + 5] == 256
    for drop in ("k3", "handover"):  # either slip leaves a piece unseen at some of the lengths, never at all of them
        missed = [n for n in E.A_LENGTHS if not visited(n, drop).all()]
        assert missed and len(missed) < len(E.A_LENGTHS), drop


@pytest.mark.parametrize("n", E.B_LENGTHS)
def test_group_b_full_chunk_and_neighbours(n):
    case = E.group_b_case(n)
    lay, want = check(case)
    last = (n + 15) // 16 - 1
    got = set((case["flip_pos"] // 16).tolist())
    assert set(range(1031)) | set(range(15350, last + 1)) <= got and len(got) == len(want) - 1 < 2400
    assert max(np.diff(sorted(got))) == 61 and np.all(case["flip_pos"] < n)
    assert not want[:-1].any() and want[-1] == 1
    assert (n > E.CHUNK) == (last == E.CHUNK // 16)  # a second chunk: one more piece
    if n % 16:
        assert unmasked_differs(lay, [len(want) - 1])


def test_group_c_every_mask_both_ways():
    case = E.group_c_case()
    lay, want = check(case)
    assert len(want) == 1920
    assert np.array_equal(want, (case["j"] >= case["v"]).astype(np.uint8))
    seen = {}
    for n, v, j, m in zip(case["lens"].tolist(), case["v"].tolist(), case["j"].tolist(), case["flip_mask"].tolist()):
        assert n % 16 == v
        seen.setdefault((n // 16, v, j), set()).add(m)
    assert seen == {(q, v, j): {0x01, 0x80} for q in E.C_Q for v in range(1, 16) for j in range(16)}
    assert unmasked_differs(lay, range(len(want)))


def test_group_d_chunks_and_pairs():
    ordered, shuffled = E.group_d_cases()
    for case in (ordered, shuffled):
        lay, want = check(case)
        assert np.all(want[case["lens"] == 0] == 1)
        assert sum(case["lens"] == 0) >= sum(case["lens"] > 0)
    assert ordered["a_len"].tolist() == list(E.D_SHAPES) and ordered["src"][0] == 0
    # the same pairs in another order, and not the same order
    key = lambda c: sorted(zip(c["src"].tolist(), c["tag"].tolist(), c["expected"].tolist()))
    assert key(ordered) == key(shuffled) and ordered["src"].tolist() != shuffled["src"].tolist()
    for s, n in enumerate(E.D_SHAPES):  # both sides of every boundary, the last byte, every chunk at once, nothing
        mine = [i for i in np.flatnonzero(ordered["src"] == s) if n]
        flips = [sorted(ordered["flip_pos"][ordered["flip_pair"] == i].tolist()) for i in mine]
        for c in range(E.CHUNK, n, E.CHUNK):
            assert [c - 1] in flips and [c] in flips
        if n:
            assert [n - 1] in flips and [] in flips
            assert any([p // E.CHUNK for p in f] == list(range((n + E.CHUNK - 1) // E.CHUNK)) and len(f) == len(set(f)) for f in flips)
    assert unmasked_differs(E.materialise(ordered), np.flatnonzero(ordered["tag"] == -1))


def test_group_e_many_small_pairs():
    case = E.group_e_case()
    lay, want = check(case)
    assert len(want) == E.E_PAIRS and set(case["lens"].tolist()) == set(range(81))
    flipped = np.zeros(E.E_PAIRS, dtype=bool)
    flipped[case["flip_pair"]] = True
    assert 0.45 < flipped.mean() < 0.55
    ignored = flipped & (want == 1)  # a flip at or past the end
    assert ignored.sum() > 10000 and np.all(case["tag"][ignored] >= case["lens"][ignored])
    assert np.all(case["tag"][flipped] < case["lens"][flipped] + 15)
    assert unmasked_differs(lay, np.flatnonzero(~flipped)[:2000])


def test_group_f_aliasing():
    (two, lay), (one, lay1), (own, lay2) = E.group_f_cases()
    check(two, lay)
    check(one, lay1)
    _, want = check(own, lay2, mixed=False)
    assert want.all() and len(want) == len(E.F_LENGTHS)
    assert lay["a"] is not lay["b"] and np.all(lay["off_a"] != lay["off_b"])
    assert lay1["a"] is lay1["b"] and np.all(lay1["off_a"] != lay1["off_b"])
    assert lay2["a"] is lay2["b"] and np.array_equal(lay2["off_a"], lay2["off_b"])
    # in one allocation no range of one side overlaps one of the other
    assert lay1["off_a"].max() + lay1["lens"].max() <= lay1["off_b"].min()


def test_staged_pass_plans():
    flips = E.lone_pair_flips()
    assert E.LONE_LEN == 5 * 32768 + 17 and len(flips) == 18 and flips[-1] is None and len(set(flips)) == 18
    assert all(0 <= p < E.LONE_LEN for p in flips[:-1])
    for c in range(E.HALF, E.LONE_LEN, E.HALF):
        assert {c - 1, c, c + 1} <= set(flips)
    plan = E.multi_pair_plan()
    assert len(plan) == 60 and {n for n, _, _ in plan} == set(E.MULTI_LENGTHS)
    assert sum(p is None for _, p, _ in plan) == 20 and all(p is None or (0 <= p < n and m) for n, p, m in plan)
    assert sum(p == n - 1 for n, p, _ in plan if p is not None and n > 1) >= 3
    # files start at many offsets within a half, and the call straddles halves many times
    assert sum(n for n, _, _ in plan) > 40 * E.HALF


def test_fill_lists():
    assert E.FILL_SPAN == 131072 and len(E.FILL_BIG_LENGTHS) == len(E.FILL_BIG_INDEX) == 19
    assert min(E.FILL_BIG_INDEX) == 1 << 32 and {n % 8 for n in E.FILL_BIG_LENGTHS} == set(range(8))
    assert E.FILL_MANY == (65535, 65536, 65540)
    lens, idx = E.fill_many(40)
    assert lens.tolist() == [i % 18 for i in range(40)] and idx.dtype == np.uint64
    assert E.fill_many(E.FILL_MANY[-1])[1].max() > 1 << 32
