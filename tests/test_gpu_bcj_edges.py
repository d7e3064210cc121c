"""The BCJ filter kernels (snappy_amd/csrc/bcj_kernels.hip) at their own edges, through snaphash_bcj_device: every input of
tests/bcj_cases.py -- the lengths around a word, a wave and a stretch, candidates in a Block's last bytes, the start
offsets, x86's eight mask states, runs of E8 over three stretches and over a whole 64 KiB tile -- as ranges of one device
buffer between canary bytes, at odd addresses, in place, in both directions, in tables of 1, 64 and 257 ranges with empty
ranges among them, against liblzma's bytes; and one dense launch of 1 MiB, whose time is printed and held against the
one-second bound DESIGN.md sec. 17 sets for any launch.  tests/test_bcj_host.py holds the same routines against the same
oracle on the CPU."""
import functools

import numpy as np
import pytest

import bcj_cases as B
from snappy_amd import Context, _lib

pytestmark = pytest.mark.gpu

GAP = 64  # canary bytes between ranges
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def want(filt, name, enc):
    data, start = next((d, s) for n, d, s in B.filter_cases(filt) if n == name)
    return B.oracle(filt, enc, data, start)


def run_table(c, filt, enc, start, items):
    """items: [(name, data)] as the ranges of one call, laid out with GAP canary bytes between them and an odd shift for
    two in three, so that ranges begin at every address class.  Every range must hold liblzma's bytes, every other byte its
    canary."""
    import torch
    offs, cur = [], GAP
    for i, (_, d) in enumerate(items):
        cur += i % 3
        offs.append(cur)
        cur += len(d) + GAP
    host = np.full(cur, CANARY, dtype=np.uint8)
    for o, (_, d) in zip(offs, items):
        host[o:o + len(d)] = np.frombuffer(d, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    c.bcj_device(filt, enc, dev.data_ptr(), np.array(offs, dtype=np.uint64), np.array([len(d) for _, d in items], dtype=np.uint64), start)
    got = dev.cpu().numpy()
    mask = np.ones(cur, dtype=bool)
    for o, (name, d) in zip(offs, items):
        assert got[o:o + len(d)].tobytes() == want(filt, name, enc), (B.NAMES[filt], name, enc, len(items))
        mask[o:o + len(d)] = False
    assert (got[mask] == CANARY).all(), (B.NAMES[filt], enc, len(items))


@pytest.mark.parametrize("enc", [True, False], ids=["encode", "decode"])
@pytest.mark.parametrize("filt", B.FILTERS, ids=lambda f: B.NAMES[f])
def test_every_case_between_canaries(snaphash_mode, filt, enc):
    with Context(device=0) as c:
        for start in sorted({s for _, _, s in B.filter_cases(filt)}):
            cases = [(n, d) for n, d, s in B.filter_cases(filt) if s == start]
            run_table(c, filt, enc, start, cases)  # all of them in one table
            small = [(n, d) for n, d in cases if len(d) < 4096]
            for k in (1, 64, 257):  # and tables of these sizes, the small cases over and over (empty ranges among them)
                run_table(c, filt, enc, start, [small[i % len(small)] for i in range(k)])
            for n, d in cases:  # the long ones alone: one range, many workgroups
                if len(d) >= 4096:
                    run_table(c, filt, enc, start, [(n, d)])
        c.bcj_device(filt, enc, 0, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))  # no range: nothing runs
        assert c.stats()["launches"] == 0


@pytest.mark.kernels_only("one launch of the kernels alone: the configuration does not enter")
def test_dense_megabyte_stays_under_a_second(snaphash_mode):
    """1 MiB of E8: no restart point behind the first byte, so one lane walks the whole range -- the longest launch a
    range of this size can make.  DESIGN.md sec. 17: no launch may take a second.  A second range of 1 MiB drawn from
    {E8, E9, 00, FF, 12} (opcode bytes everywhere, candidates among them) rides in the same table."""
    import torch
    n = 1 << 20
    run = b"\xE8" * n
    dense = B.x86_dense(n, 12)
    host = np.frombuffer(run + dense, dtype=np.uint8).copy()
    with Context(device=0) as c:
        for enc in (True, False):
            dev = torch.from_numpy(host).cuda()
            torch.cuda.synchronize()
            c.bcj_device("x86", enc, dev.data_ptr(), np.array([0, n], dtype=np.uint64), np.array([n, n], dtype=np.uint64))
            st = c.stats()
            print("bcj dense 1 MiB + 1 MiB, %s: %.3f ms in %d launches" % ("encode" if enc else "decode", st["kernel_ms"], st["launches"]))
            assert st["launches"] == 2 and 0 < st["kernel_ms"] < 1000.0, st
            got = dev.cpu().numpy()
            assert got[:n].tobytes() == B.oracle(B.X86, enc, run)
            assert got[n:].tobytes() == B.oracle(B.X86, enc, dense)


@pytest.mark.kernels_only("argument checks: the configuration does not enter")
def test_refusals(snaphash_mode):
    import torch
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    one = np.array([0], dtype=np.uint64), np.array([64], dtype=np.uint64)
    with Context(device=0) as c:
        for filt, start in ((0, 0), (3, 0), (5, 0), (9, 0), (0x21, 0), (7, 2), (7, 1), (8, 1)):
            with pytest.raises(_lib.SnaphashError) as e:
                c.bcj_device(filt, True, dev.data_ptr(), *one, start)
            assert e.value.code == _lib.EINVAL, (filt, start)
        c.bcj_device(8, True, dev.data_ptr(), *one, 2)  # Thumb's alignment is 2
        assert (dev.cpu().numpy() == 0).all()
