"""sha512_wide_kernel, sha512_split_kernel<false>, sha512_split_kernel<true> (PAIR) and its staged twin
(snappy_amd/csrc/sha512_kernels.hip) at their own edges: each alone over job tables built by hand, through
snaphash_sha512_jobs_device.  Every table the product builds is sorted longest first, hashes streams far below 4 GiB and
is checked by its final digests only; here any stream sits on any lane, a stream's byte count is whatever Job.total_prev
can hold, and after every launch every row of both arrays is looked at: the rows a job names against hashlib or the
plain-Python reference (tests/sha512_ref.py), all others, the 4 KiB around the arrays and the input against what was
there before.  "Lane" below is a job's index in the table mod 64 -- the stream's place in its workgroup."""
import hashlib

import numpy as np
import pytest

import sha512_ref as ref
from test_core_host import TAIL_BYTES, TOTAL_PREV

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("one kernel a launch, named by the test")]

N = 1 << 20
CANARY = 4096
FIRST, FINAL = 1, 2
# tails around the padding's two block counts (111 | 112) and the block, with none, one and two blocks before them
T = [0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 255, 256]
KERNELS = [("wide", False), ("split", False), ("pair", False)]
KERNELS_AND_STAGED = KERNELS + [("pair", True)]


def ids(k):
    return k[0] + ("-staged" if k[1] else "")


@pytest.fixture(scope="module")
def c512(built_lib):
    from snappy_amd import Context, _lib
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def buf():
    """Random bytes in HBM, twice (the second copy is what the first is compared with after a launch), and on the host."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    host = np.random.default_rng(512).integers(0, 256, N, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    keep = dev.clone()
    torch.cuda.synchronize()
    assert dev.data_ptr() % 16 == 0
    return host.tobytes(), dev, keep


def place(lens):
    """Every stream at a 16-aligned offset of its own, 16 bytes or more of the buffer's random bytes between two: the
    16-byte piece a kernel fetches past a stream's end holds non-zero bytes that belong to no stream."""
    offs, o = [], 16
    for n in lens:
        offs.append(o)
        o += (n + 15) // 16 * 16 + 16
    assert o <= N
    return offs


def state_row(H):
    return np.frombuffer(b"".join(x.to_bytes(8, "little") for x in H), dtype=np.uint8)


def row_state(row):
    return [int.from_bytes(row[8 * k:8 * k + 8].tobytes(), "little") for k in range(8)]


_sha = {}


def sha(data, o, n):
    if (o, n) not in _sha:
        _sha[(o, n)] = np.frombuffer(hashlib.sha512(data[o:o + n]).digest(), dtype=np.uint8)
    return _sha[(o, n)]


def kernel_id(name):
    from snappy_amd import _lib
    return {"wide": _lib.KERNEL_WIDE, "split": _lib.KERNEL_SPLIT, "pair": _lib.KERNEL_PAIR}[name]


def check(c, kern, buf, jobs, want, state, digs):
    """One launch of `kern` over jobs -- (offset in the buffer, nbytes, total_prev, idx, flags), in this order -- with the
    state and digest arrays (numpy uint8, rows x 64: what the device holds before) between canaries; want[i] is the 64
    bytes job i must leave in its row (digest row if final, state row if not).  Asserts that nothing else changed and
    leaves the launch's results in state and digs, for a next launch to carry on from."""
    import torch
    data, dev, keep = buf
    name, staged = kern
    rows = state.shape[0]
    assert state.shape == digs.shape == (rows, 64) and len(want) == len(jobs)
    assert all(o % 16 == 0 and o + (n + 15) // 16 * 16 <= N for o, n, _, _, _ in jobs)
    fill = np.random.default_rng(rows).integers(1, 256, 2 * CANARY, dtype=np.uint8)
    host = [np.concatenate([fill[:CANARY], a.reshape(-1), fill[CANARY:]]) for a in (state, digs)]
    d_arr = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    c.sha512_jobs_device(kernel_id(name), [(dev.data_ptr() + o, n, tp, idx, fl) for o, n, tp, idx, fl in jobs], rows,
                         d_arr[0].data_ptr() + CANARY, d_arr[1].data_ptr() + CANARY, staged=staged)
    got = [a.cpu().numpy() for a in d_arr]
    assert torch.equal(dev, keep), "the input was written"
    for g, h, what in zip(got, host, ("state", "digests")):
        assert (g[:CANARY] == h[:CANARY]).all() and (g[-CANARY:] == h[-CANARY:]).all(), "bytes around the %s array were written" % what
    new_state, new_digs = (g[CANARY:-CANARY].reshape(rows, 64) for g in got)
    exp_state, exp_digs = state.copy(), digs.copy()
    for (_, _, _, idx, fl), w in zip(jobs, want):
        (exp_digs if fl & FINAL else exp_state)[idx] = w
    where = {j[3]: (i, i % 64) + tuple(j[1:]) for i, j in enumerate(jobs)}  # row -> table slot, lane, the job
    for new, exp, what in ((new_state, exp_state, "state"), (new_digs, exp_digs, "digest")):
        bad = np.flatnonzero((new != exp).any(axis=1))
        assert bad.size == 0, "%s rows differ: %s" % (what, [(int(r), where.get(int(r), "named by no job")) for r in bad[:6]])
    state[:], digs[:] = new_state, new_digs


def fresh(rows):
    """Sentinel rows: a state row a job must not read or write, a digest row before its digest."""
    return np.full((rows, 64), 0xC3, dtype=np.uint8), np.full((rows, 64), 0x5A, dtype=np.uint8)


def whole_streams(c, kern, buf, lens):
    """Every stream whole, first | final, stream s at table slot s and row s."""
    offs = place(lens)
    jobs = [(o, n, 0, s, FIRST | FINAL) for s, (o, n) in enumerate(zip(offs, lens))]
    check(c, kern, buf, jobs, [sha(buf[0], o, n) for o, n in zip(offs, lens)], *fresh(len(lens)))


# ---- a. every tail class at every lane ------------------------------------------------------------------------------

@pytest.mark.parametrize("kern", KERNELS, ids=ids)
def test_every_tail_class_at_every_lane(c512, buf, kern):
    for r in range(len(T)):
        whole_streams(c512, kern, buf, [T[(s + r) % len(T)] for s in range(64)])


# ---- b. block counts out of order -----------------------------------------------------------------------------------

BITREV = [int("{:06b}".format(s)[::-1], 2) for s in range(64)]
ORDERS = {"ascending": list(range(64)), "descending": list(range(63, -1, -1)), "bit_reversed": BITREV}


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("kern", KERNELS, ids=ids)
def test_block_counts_out_of_order(c512, buf, kern, order):
    """0..63 blocks and a tail on the 64 lanes of one workgroup, the longest stream last, first, or anywhere: every
    residue of the helpers' even/odd split and of the ring of three ends on some lane while others go on."""
    whole_streams(c512, kern, buf, [128 * ORDERS[order][s] + (5, 111, 112, 127)[s % 4] for s in range(64)])


@pytest.mark.parametrize("k", [0, 3, 4, 7, 8, 31, 32, 35, 36, 63])
@pytest.mark.parametrize("kern", KERNELS, ids=ids)
def test_one_long_stream_among_empty_ones(c512, buf, kern, k):
    """Lane k alone decides how long the workgroup runs; the 63 empty streams end in the first block-time and ride along
    for 40 more.  The lanes are both roles of PAIR's lane mapping (k & 7 below 4, and not) in both of its round waves."""
    whole_streams(c512, kern, buf, [128 * 40 + 5 if s == k else 0 for s in range(64)])


# ---- c. table sizes -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 16384, 16385])
@pytest.mark.parametrize("kern", KERNELS, ids=ids)
def test_table_sizes(c512, buf, kern, n):
    """Around PAIR's round wave (32 streams), the workgroup (64) and two of them; 16 384 is a workgroup on each of the 256
    CUs, 16 385 one more.  Streams overlap in the buffer (it is only read); rows run against the table's order."""
    data, _, _ = buf
    lens = [100 + (37 * i) % 300 for i in range(n)]
    offs = [16 + 48 * (i % 20000) for i in range(n)]
    jobs = [(o, ln, 0, n - 1 - i, FIRST | FINAL) for i, (o, ln) in enumerate(zip(offs, lens))]
    check(c512, kern, buf, jobs, [sha(data, o, ln) for o, ln in zip(offs, lens)], *fresh(n))


# ---- d. carried state -----------------------------------------------------------------------------------------------

def carried_plan():
    """96 streams in 128 rows over three launches.  -> (offs, lens, idx, launches); a launch is a list of
    (stream, from byte, to byte, final) in table order.  The cuts, by i % 7 (with what a short stream falls back to):
      0  whole in launch 0
      1  whole in launch 1
      2  launch 0: a first part; launch 1: the rest                           (no full block: as 0)
      3  launch 0, 1: a part each; launch 2: the rest                         (fewer than two full blocks: as 2)
      4  launch 0: every full block; launch 2: the tail, 0 bytes for some     (no full block: as 1)
      5  launch 1: a first part; launch 2: the rest                           (no full block: as 1)
      6  whole in launch 2"""
    lens = [128 * (i % 9) + T[i % 12] for i in range(96)]
    idx = [(37 * i + 5) % 128 for i in range(96)]
    launches = [[], [], []]
    for i, n in enumerate(lens):
        full, kind = n // 128, i % 7
        if kind == 3 and full < 2:
            kind = 2
        if kind == 2 and full < 1:
            kind = 0
        if kind in (4, 5) and full < 1:
            kind = 1
        if kind in (0, 1, 6):
            launches[(0, 1, None, None, None, None, 2)[kind]].append((i, 0, n, True))
        elif kind in (2, 5):
            cut = 128 * max(1, full // 2)
            launches[0 if kind == 2 else 1].append((i, 0, cut, False))
            launches[1 if kind == 2 else 2].append((i, cut, n, True))
        elif kind == 3:
            c1 = 128 * max(1, full // 3)
            c2 = c1 + 128 * max(1, (full - full // 3) // 2)
            launches[0].append((i, 0, c1, False))
            launches[1].append((i, c1, c2, False))
            launches[2].append((i, c2, n, True))
        else:
            launches[0].append((i, 0, 128 * full, False))
            launches[2].append((i, 128 * full, n, True))
    rng = np.random.default_rng(96)
    launches = [[la[j] for j in rng.permutation(len(la))] for la in launches]  # block counts in no order on the lanes
    return place(lens), lens, idx, launches


_chain = {}


def chain(data, off, upto):
    """The chaining value after the first `upto` bytes (whole blocks) of the stream at off, from the one before it."""
    if upto == 0:
        return ref.IV
    if (off, upto) not in _chain:
        prev = max([u for o, u in _chain if o == off and u < upto], default=0)
        _chain[(off, upto)] = ref.segment(chain(data, off, prev), data[off + prev:off + upto], prev, False)
    return _chain[(off, upto)]


def test_the_carried_plan_mixes_every_kind_of_job():
    """What test_carried_state_after_every_launch relies on (no GPU in this one)."""
    offs, lens, idx, launches = carried_plan()
    assert len(set(idx)) == 96 and max(idx) < 128  # 32 rows are named by no stream
    at = [0] * 96
    for la in launches:  # a stream's segments follow one another, all but the last whole blocks, and it ends once, at its end
        for s, a, b, fin in la:
            assert a == at[s] and (b == lens[s] if fin else (b - a) % 128 == 0 and b > a)
            at[s] = -1 if fin else b
        assert len({s for s, _, _, _ in la}) == len(la)
    assert at == [-1] * 96
    kinds = [{(a == 0, fin) for s, a, b, fin in la} for la in launches]  # (first, final)
    assert kinds[0] == {(True, True), (True, False)}
    assert kinds[1] == {(True, True), (True, False), (False, True), (False, False)}
    assert kinds[2] == {(True, True), (False, True)}
    tails = {b - a for la in launches for s, a, b, fin in la if a > 0 and fin}
    assert {0, 111, 112, 127} <= tails  # continued + final: nothing left, and the padding's block layouts
    assert any(b == lens[s] and not fin for la in launches for s, a, b, fin in la)  # (the 0 bytes follow whole blocks)
    assert all(32 < len(la) < 96 for la in launches)  # streams absent from every launch; both of PAIR's round waves busy


@pytest.mark.parametrize("kern", KERNELS_AND_STAGED, ids=ids)
def test_carried_state_after_every_launch(c512, buf, kern):
    """A stream in up to three segments: after EACH launch the state row of every job that is not final is the reference's
    chaining value, every final job's digest is hashlib's, a final job's state row and any other job's digest row are as
    before -- as are the 32 rows no stream has and the rows of streams absent from the launch."""
    data = buf[0]
    offs, lens, idx, launches = carried_plan()
    state, digs = fresh(128)
    for la in launches:
        jobs, want = [], []
        for s, a, b, fin in la:
            jobs.append((offs[s] + a, b - a, a, idx[s], (FIRST if a == 0 else 0) | (FINAL if fin else 0)))
            want.append(sha(data, offs[s], lens[s]) if fin else state_row(chain(data, offs[s], b)))
        check(c512, kern, buf, jobs, want, state, digs)


# ---- e. large totals ------------------------------------------------------------------------------------------------

_large = []


def large_cases(data):
    """(offset, nbytes, total_prev, flags, state row before, 64 bytes wanted): every byte count of TOTAL_PREV before every
    tail of TAIL_BYTES, continued and final from a state row of random bytes; and where the tail is whole blocks, once
    more as a job that is not final (the count plays no part then)."""
    if not _large:
        rng = np.random.default_rng(61)
        combos = [(tp, n, FINAL) for tp in TOTAL_PREV for n in TAIL_BYTES] + [(tp, n, 0) for tp in TOTAL_PREV for n in TAIL_BYTES if n % 128 == 0]
        for (tp, n, fl), o in zip(combos, place([n for _, n, _ in combos])):
            row = rng.integers(0, 256, 64, dtype=np.uint8)
            H = ref.segment(row_state(row), data[o:o + n], tp, bool(fl & FINAL))
            _large.append((o, n, tp, fl, row, np.frombuffer(ref.digest(H), dtype=np.uint8) if fl & FINAL else state_row(H)))
    return _large


@pytest.mark.parametrize("reverse", [False, True], ids=["table_order", "reversed"])
@pytest.mark.parametrize("kern", KERNELS, ids=ids)
def test_large_totals(c512, buf, kern, reverse):
    """The padding's 128-bit length from a 64-bit byte count: totals past 2^32 bits, 2^32 bytes, 2^35 bytes, and at and
    above 2^61 bytes, where the count's top bits enter the length's high word (no caller reaches those; the kernels
    compute them all the same)."""
    cases = large_cases(buf[0])
    order = list(range(len(cases)))[::-1] if reverse else list(range(len(cases)))
    state, digs = fresh(len(cases))
    for i, case in enumerate(cases):
        state[i] = case[4]
    jobs = [(cases[i][0], cases[i][1], cases[i][2], i, cases[i][3]) for i in order]
    check(c512, kern, buf, jobs, [cases[i][5] for i in order], state, digs)


# ---- f. refusals ----------------------------------------------------------------------------------------------------

def test_refusals(c512, buf):
    import torch
    from snappy_amd import Context, SnaphashError, _lib
    data, dev, _ = buf
    rows = torch.zeros(2 * 4 * 64, dtype=torch.uint8, device="cuda")
    d_state, d_digs, base = rows.data_ptr(), rows.data_ptr() + 4 * 64, dev.data_ptr()
    good = [(base + 16, 300, 0, 0, FIRST | FINAL), (base + 512, 128, 0, 1, FIRST)]

    def refused(kernel, jobs, n_rows=4, state=d_state, digs=d_digs):
        with pytest.raises(SnaphashError) as e:
            c512.sha512_jobs_device(kernel, jobs, n_rows, state, digs)
        assert e.value.code == _lib.EINVAL, e.value

    for kernel in (_lib.KERNEL_AUTO, 5, 0xffffffff):
        refused(kernel, good)
    try:
        Context(kernel=_lib.KERNEL_QUAD, flags=_lib.FLAG_GPU_ONLY).close()
    except SnaphashError:
        refused(_lib.KERNEL_QUAD, good)                               # a build without it (the default)
    for k in (_lib.KERNEL_WIDE, _lib.KERNEL_SPLIT, _lib.KERNEL_PAIR):
        refused(k, [(base + 8, 300, 0, 0, FIRST | FINAL)])            # the address
        refused(k, [(base, 1 << 35, 0, 0, FIRST | FINAL)])            # 32 GiB
        refused(k, good + [(base, 100, 0, 2, FIRST)])                 # not final, not whole blocks
        refused(k, good + [(base, 128, 128, 2, 0), (base, 129, 128, 3, 0)])
        refused(k, good + [(base, 0, 0, 2, FIRST)])                   # first, not final, empty
        refused(k, good + [(base, 0, 0, 4, FIRST | FINAL)])           # idx is no row
        refused(k, good, n_rows=1)
        refused(k, good + [(base, 0, 0, 1, FIRST | FINAL)])           # one row twice
        refused(k, good + [(base, 0, 0, 2, 4)])                       # an unknown flag
        refused(k, good, state=d_state + 4)
        refused(k, good, digs=d_digs + 8)
    b = _lib.Batch(c512, 1)
    try:
        refused(_lib.KERNEL_WIDE, good)                               # a streaming batch is open
    finally:
        b.abort()
    assert (rows.cpu().numpy() == 0).all()                            # a refused table launches nothing
    c512.sha512_jobs_device(_lib.KERNEL_WIDE, [], 0, 0, 0)            # no jobs: nothing to do
    for kern in KERNELS:                                              # and the context still hashes
        whole_streams(c512, kern, buf, [300, 0, 129])
