"""ranges_equal_kernel (sha512_kernels.hip), launch_compare_ranges and the staged pass of files_equal_impl
(snaphash_api.cpp) at their own edges: the cases of tests/cmp_edge_cases.py through Context.ranges_equal_device and
Context.files_equal, the whole verdict vector against the cases' closed form (tests/test_cmp_edges_host.py shows on
the CPU that it is what a plain byte compare gives).  The answer that must never come out wrong is a false "equal".
All of it in the GPU-only configuration: the HBM-resident entry point never plans, and the default configuration
would compare files of this size on host threads.  At the end fill_synthetic_kernel, which writes the content of every
full-size test and of the benchmark, at its grid-stride loop and at the slicing of its file list, byte for byte against
the oracle's generator and the Python one."""
import numpy as np
import pytest

import cmp_edge_cases as E

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("the compare and fill kernels themselves: every byte through them")]

PAD = 4096
CANARY = 0x5A


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


@pytest.fixture(scope="module")
def cmp_ctx(built_lib):
    """One context for the file: the compare kernel does not depend on the SHA-512 variant."""
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


def verdicts(c, case, lay, a, b):
    """One call; the verdict bytes lie between canaries and start out as neither 0 nor 1.  -> None or what is wrong."""
    torch = _torch()
    n = len(lay["lens"])
    assert E.in_bounds(lay, a.numel(), b.numel()), case["name"]
    eq = torch.full((PAD + n + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # the ctx stream is non-blocking: order it after torch's fills and copies
    c.ranges_equal_device(a.data_ptr(), lay["off_a"], b.data_ptr(), lay["off_b"], lay["lens"], eq.data_ptr() + PAD)
    c.sync()
    e = eq.cpu().numpy()
    if not ((e[:PAD] == CANARY).all() and (e[PAD + n:] == CANARY).all()):
        return (case["name"], "a byte around the verdicts was written")
    got = e[PAD:PAD + n]
    if not np.array_equal(got, case["expected"]):
        return (case["name"], "(length, index, got, want)", E.report(case, got))
    return None


def run(c, case, lay=None):
    torch = _torch()
    lay = lay or E.materialise(case)
    a = torch.from_numpy(lay["a"]).cuda()
    b = a if lay["b"] is lay["a"] else torch.from_numpy(lay["b"]).cuda()
    return verdicts(c, case, lay, a, b)


def test_group_a_every_piece_around_the_loop_bounds(cmp_ctx):
    """The unrolled loop's `p + 768 < nwhole`, its hand-over of p to the stride-256 loop and `p < npieces`: at every
    length one variant per 16-byte piece differs in that piece alone, so a piece no lane looks at is a false "equal";
    the one lane that sees it sits in each of the four waves in turn (`__any` and the store of the wave's lane 0)."""
    wrong = [w for w in (run(cmp_ctx, E.group_a_case(n)) for n in E.A_LENGTHS) if w]
    assert not wrong, wrong[:4]


def test_group_b_full_chunk_and_neighbours(cmp_ctx):
    """A chunk of exactly kCmpChunk, one of 16 383 whole pieces and 3 bytes, and a second chunk of a single byte.  A
    and B are built in HBM; torch's own compare of the same bytes stands beside the closed form."""
    torch = _torch()
    for n in E.B_LENGTHS:
        case = E.group_b_case(n)
        k, stride, oa = len(case["src"]), E.pad16(n) + E.SLACK, int(case["a_off"][0])
        a = torch.from_numpy(case["a"]).cuda()
        b = torch.full((k, stride), E.FILL_B, dtype=torch.uint8, device="cuda")
        b[:, :n] = a[oa:oa + n]
        rows, cols = torch.from_numpy(case["flip_pair"]).cuda(), torch.from_numpy(case["flip_pos"]).cuda()
        b[rows, cols] = b[rows, cols] ^ torch.from_numpy(case["flip_mask"]).cuda()
        same = ~(b[:, :n] != a[oa:oa + n]).any(1)
        assert np.array_equal(same.cpu().numpy().astype(np.uint8), case["expected"]), n
        del same
        u = lambda x: np.ascontiguousarray(x, dtype=np.uint64)
        lay = dict(off_a=u(np.full(k, oa)), off_b=u(np.arange(k) * stride), lens=u(np.full(k, n)))
        wrong = verdicts(cmp_ctx, case, lay, a, b.view(-1))
        assert not wrong, wrong
        del a, b


def test_group_c_tail_mask(cmp_ctx):
    """`valid = nbytes & 15` and the mask of each dword (nv <= 0, nv < 4, whole): for every count of valid bytes the
    last valid byte counts and the first invalid one does not, low bit and high bit, with the last piece in the
    stride-256 loop's first step, after whole pieces, and after a trip of the unrolled loop."""
    wrong = run(cmp_ctx, E.group_c_case())
    assert not wrong, wrong


def test_group_d_chunks_and_pair_mapping(cmp_ctx):
    """launch_compare_ranges' chunk table: no chunk for an empty pair, several for a long one, and ch.pair naming the
    verdict byte; a difference on either side of every chunk boundary; empty pairs stay "equal"."""
    wrong = [w for w in (run(cmp_ctx, case) for case in E.group_d_cases()) if w]
    assert not wrong, wrong


def test_group_e_many_small_pairs(cmp_ctx):
    """200 000 chunks of at most 80 bytes in one launch; flips past a pair's end are ignored."""
    wrong = run(cmp_ctx, E.group_e_case())
    assert not wrong, wrong


def test_group_f_aliasing(cmp_ctx):
    """Both sides in one allocation at different offsets, a range against itself, and two bases with off_a != off_b
    for every pair."""
    wrong = [w for w in (run(cmp_ctx, case, lay) for case, lay in E.group_f_cases()) if w]
    assert not wrong, wrong


# ---- the staged pass ----------------------------------------------------------------------------------------------------

def _w(path, data):
    with open(path, "wb") as f:
        f.write(data)


def staged_ctx():
    from snappy_amd import Context, _lib
    return Context(staging_bytes=E.STAGING, flags=_lib.FLAG_GPU_ONLY)


def test_staged_lone_pair_cut_into_segments(built_lib, tmp_path):
    """files_equal_impl with staging_bytes = 64 KiB: H = (slot_want / 2) & ~255 = 32 768, so a lone pair of
    5 * 32 768 + 17 bytes is compared as six segments across the two alternating halves (six launches), and a
    segment's verdict is AND-ed in when its half is retired.  One flipped bit per call, at the file's ends and on
    both sides of every cut: a lost verdict of any segment is a false "equal"."""
    rng = np.random.default_rng(0x10E)
    data = rng.integers(0, 256, size=E.LONE_LEN, dtype=np.uint8)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    _w(a, data.tobytes())
    wrong = []
    with staged_ctx() as c:
        for pos in E.lone_pair_flips():
            other = data.copy()
            if pos is not None:
                other[pos] ^= 1 << (pos % 8)
            _w(b, other.tobytes())
            got = c.files_equal([(a, b)])
            assert c.stats()["launches"] == (E.LONE_LEN + E.HALF - 1) // E.HALF == 6
            if got != [pos is None]:
                wrong.append((pos, got))
    assert not wrong, wrong


def test_staged_many_pairs_and_buffer_reuse(built_lib, oracle, tmp_path):
    """Sixty pairs through halves of 32 KiB: files start at every kind of offset within a half and straddle halves
    many times.  The oracle's FilesAreEqual says what is equal; the same ctx then takes the list reversed: a verdict
    follows its pair, not the slot it was staged in."""
    rng = np.random.default_rng(0x3A)
    pairs = []
    for i, (n, pos, mask) in enumerate(E.multi_pair_plan()):
        data = rng.integers(0, 256, size=n, dtype=np.uint8)
        a, b = str(tmp_path / ("a%d" % i)), str(tmp_path / ("b%d" % i))
        _w(a, data.tobytes())
        if pos is not None:
            data[pos] ^= mask
        _w(b, data.tobytes())
        pairs.append((a, b))
    want = [oracle.files_equal(a, b) for a, b in pairs]
    assert want == [pos is None for _, pos, _ in E.multi_pair_plan()] and sum(want) == 20
    total = sum(n for n, _, _ in E.multi_pair_plan())
    with staged_ctx() as c:
        for order in (pairs, pairs[::-1]):
            got = c.files_equal(order)
            exp = want if order is pairs else want[::-1]
            assert got == exp, [(order[i][0], got[i]) for i in range(len(got)) if got[i] != exp[i]][:8]
            assert c.stats()["launches"] >= total // E.HALF


# ---- fill_synthetic_kernel ----------------------------------------------------------------------------------------------

def filled(c, lens, idx):
    """-> the files' region after one fill (offsets 8-byte aligned, end to end); what lies around it is untouched."""
    torch = _torch()
    from snappy_amd import synthetic
    lens, idx = np.ascontiguousarray(lens, dtype=np.uint64), np.ascontiguousarray(idx, dtype=np.uint64)
    off, total = synthetic.pack_offsets(lens, 8)
    dev = torch.full((PAD + total + PAD,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    c.fill_synthetic_device(dev.data_ptr() + PAD, off, lens, idx)
    c.sync()
    got = dev.cpu().numpy()
    assert (got[:PAD] == CANARY).all() and (got[PAD + total:] == CANARY).all()
    return off, got[PAD:PAD + total]


def generated(make, off, lens, idx, total):
    want = np.full(total, CANARY, dtype=np.uint8)
    for o, n, i in zip(off.tolist(), np.asarray(lens).tolist(), np.asarray(idx).tolist()):
        want[o:o + n] = np.frombuffer(make(n, i), dtype=np.uint8) if n else 0
    return want


def first_wrong(got, want, off):
    bad = np.flatnonzero(got != want)
    return None if not len(bad) else ("file", int(np.searchsorted(off, bad[0], side="right") - 1), "byte", int(bad[0]))


def test_fill_grid_stride_loop(cmp_ctx, oracle):
    """Files above 64 blocks x 256 words = 128 KiB take more than one step of the grid-stride loop: lengths around
    that span and its multiples, every tail length, file indices at and above 2**32."""
    from snappy_amd import synthetic
    lens, idx = np.array(E.FILL_BIG_LENGTHS, dtype=np.uint64), np.array(E.FILL_BIG_INDEX, dtype=np.uint64)
    off, got = filled(cmp_ctx, lens, idx)
    for make in (lambda n, i: oracle.fill_synthetic(n, i).tobytes(), synthetic.file_bytes):
        assert first_wrong(got, generated(make, off, lens, idx, len(got)), off) is None


_many = {}


def test_fill_file_list_slices(cmp_ctx, oracle):
    """gridDim.y = 65 535 files per launch: lists of exactly one slice, one file more, and a few more, lengths
    0..17 (the bytes between two files are the neighbour's or nobody's)."""
    from snappy_amd import synthetic
    for n in E.FILL_MANY:
        lens, idx = E.fill_many(n)
        off, got = filled(cmp_ctx, lens, idx)
        if not _many:  # the longer lists start with the shorter ones: generate once, for the longest
            ml, mi = E.fill_many(max(E.FILL_MANY))
            mo, mt = synthetic.pack_offsets(ml, 8)
            _many["oracle"] = generated(lambda k, i: oracle.fill_synthetic(k, i).tobytes(), mo, ml, mi, mt)
            _many["python"] = generated(synthetic.file_bytes, mo, ml, mi, mt)
        for want in _many.values():
            assert first_wrong(got, want[:len(got)], off) is None, n
