"""The PowerPC, IA64, SPARC and Delta filter kernels (snappy_amd/csrc/bcj_kernels.hip, delta_kernels.hip) at their own edges,
through snaphash_xz_filter_device: every input of tests/xzfilt_cases.py -- the lengths around a word, a bundle, a stretch and
a 64 KiB tile, candidates in a Block's last unit and in its trailing partial unit, the start offsets, every IA64 template,
both SPARC sign forms, PowerPC targets that wrap 2^26; Delta at distances 1 .. 256 over lengths around a distance and a
tile, random bytes and the all-0x01 inputs that show a lost carry -- as ranges of one device buffer between canary bytes, at
odd addresses, in place, in both directions, in tables of 1, 64 and 257 ranges with empty ranges among them, against
liblzma's bytes; the three-tile Delta cases alone, so that carries cross workgroups; the largest launch's time, printed and
held against the one-second bound DESIGN.md sec. 17 sets for any launch; and the refusals.  tests/test_xzfilt_host.py holds
the same routines against the same oracle on the CPU."""
import numpy as np
import pytest

import xzfilt_cases as F
from snappy_amd import Context, _lib

pytestmark = pytest.mark.gpu

GAP = 64  # canary bytes between ranges
CANARY = 0xA5


def run_table(c, filt, enc, param, items):
    """items: [(name, data)] as the ranges of one call, laid out with GAP canary bytes between them and an odd shift for
    two in three, so that ranges begin at every address class.  param: a BCJ filter's start_offset, Delta's distance.  Every
    range must hold liblzma's bytes, every other byte its canary.  -> the call's stats"""
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
    lens = np.array([len(d) for _, d in items], dtype=np.uint64)
    if filt == F.DELTA:
        c.xz_filter_device(filt, enc, dev.data_ptr(), np.array(offs, dtype=np.uint64), lens, param=param)
    else:
        c.xz_filter_device(filt, enc, dev.data_ptr(), np.array(offs, dtype=np.uint64), lens, param)
    st = c.stats()
    got = dev.cpu().numpy()
    mask = np.ones(cur, dtype=bool)
    for o, (name, d) in zip(offs, items):
        assert got[o:o + len(d)].tobytes() == F.oracle(filt, enc, d, param), (F.NAMES[filt], name, enc, len(items))
        mask[o:o + len(d)] = False
    assert (got[mask] == CANARY).all(), (F.NAMES[filt], enc, len(items))
    return st


def run_tables(c, filt, enc, param, cases):
    """all of them in one table; tables of 1, 64 and 257 ranges, the small cases over and over (empty ranges among them);
    the long ones alone: one range, many workgroups"""
    run_table(c, filt, enc, param, cases)
    small = [(n, d) for n, d in cases if len(d) < 4096]
    for k in (1, 64, 257):
        run_table(c, filt, enc, param, [small[i % len(small)] for i in range(k)])
    for n, d in cases:
        if len(d) >= 4096:
            run_table(c, filt, enc, param, [(n, d)])


@pytest.mark.parametrize("enc", [True, False], ids=["encode", "decode"])
@pytest.mark.parametrize("filt", F.WORD_FILTERS, ids=lambda f: F.NAMES[f])
def test_every_word_case_between_canaries(snaphash_mode, filt, enc):
    with Context(device=0) as c:
        for start in sorted({s for _, _, s in F.word_cases(filt)}):
            run_tables(c, filt, enc, start, [(n, d) for n, d, s in F.word_cases(filt) if s == start])
        c.xz_filter_device(filt, enc, 0, np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64))  # no range: nothing runs
        assert c.stats()["launches"] == 0


@pytest.mark.parametrize("enc", [True, False], ids=["encode", "decode"])
@pytest.mark.parametrize("d", F.DISTS)
def test_every_delta_case_between_canaries(snaphash_mode, d, enc):
    """The cases of one distance; those of more than two tiles run in test_three_tiles_alone."""
    cases = [(n, data) for n, data, dist in F.delta_cases() if dist == d and len(data) <= 2 * F.TILE]
    with Context(device=0) as c:
        run_tables(c, F.DELTA, enc, d, cases)
        st = run_table(c, F.DELTA, enc, d, cases[:3])
        assert st["launches"] == (2 if enc else 3) and st["kernel_ms"] > 0, st
        run_table(c, F.DELTA, enc, d, [("empty", b"")] * 3)  # empty ranges alone: nothing runs
        assert c.stats()["launches"] == 0


@pytest.mark.kernels_only("one launch of the kernels alone: the configuration does not enter")
@pytest.mark.parametrize("enc", [True, False], ids=["encode", "decode"])
def test_three_tiles_alone(snaphash_mode, enc):
    """3 x 65 536 + d + 1 bytes as the call's one range: four workgroups, and a carry (decode) or a saved tail (encode) from
    each to the next.  Random bytes at every distance, all-0x01 at 3 and 255 (xzfilt_cases.py says why)."""
    with Context(device=0) as c:
        for name, data, d in F.three_tile_delta_cases():
            run_table(c, F.DELTA, enc, d, [(name, data)])
        # and two such ranges with a one-tile range and an empty one between them: a range's carries stay its own
        ones = [(n, data) for n, data, d in F.three_tile_delta_cases() if d == 255]
        run_table(c, F.DELTA, enc, 255, [ones[0], ("short", F.rnd(700, 5)), ("empty", b""), ones[1]])


@pytest.mark.kernels_only("one launch of the kernels alone: the configuration does not enter")
def test_largest_launches_stay_under_a_second(snaphash_mode):
    """2 MiB as one range -- 32 tiles, the carry kernel's longest walk of the suite -- through Delta at d = 1, 3 and 256 and
    through each word filter on dense candidates.  DESIGN.md sec. 17: no launch may take a second; the call's time bounds
    each of its launches."""
    import torch
    n = 2 << 20
    one = np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64)
    data = F.rnd(n, 77)
    host = np.frombuffer(data, dtype=np.uint8)
    with Context(device=0) as c:
        for filt, param in [(F.DELTA, 1), (F.DELTA, 3), (F.DELTA, 256)] + [(f, 0) for f in F.WORD_FILTERS]:
            src = host if filt == F.DELTA else np.frombuffer(F.dense(filt, n, 5), dtype=np.uint8)
            for enc in (True, False):
                dev = torch.from_numpy(src.copy()).cuda()
                torch.cuda.synchronize()
                c.xz_filter_device(filt, enc, dev.data_ptr(), *one, param=param)
                st = c.stats()
                print("%s %d, 2 MiB, %s: %.3f ms in %d launches" % (F.NAMES[filt], param, "encode" if enc else "decode", st["kernel_ms"], st["launches"]))
                assert 0 < st["kernel_ms"] < 1000.0, st
                assert st["launches"] == ((2 if enc else 3) if filt == F.DELTA else 1), st
                assert dev.cpu().numpy().tobytes() == F.oracle(filt, enc, src.tobytes(), param)


@pytest.mark.kernels_only("argument checks: the configuration does not enter")
def test_refusals(snaphash_mode):
    import torch
    dev = torch.zeros(64, dtype=torch.uint8, device="cuda")
    one = np.array([0], dtype=np.uint64), np.array([64], dtype=np.uint64)
    with Context(device=0) as c:
        bad = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (10, 0, 0), (11, 0, 0), (0x21, 0, 0),  # ids
               (3, 0, 0), (3, 0, 257), (3, 0, 0xFFFFFFFF), (3, 4, 1),                   # Delta: a bad distance, a start_offset
               (4, 0, 1), (5, 0, 4), (9, 0, 1),                                         # a param on a BCJ id
               (5, 2, 0), (6, 8, 0), (6, 4, 0), (9, 2, 0), (7, 2, 0), (8, 1, 0)]        # a start_offset off the alignment
        for filt, start, param in bad:
            with pytest.raises(_lib.SnaphashError) as e:
                c.xz_filter_device(filt, True, dev.data_ptr(), *one, start, param)
            assert e.value.code == _lib.EINVAL, (filt, start, param)
        assert (dev.cpu().numpy() == 0).all()  # touching nothing
        c.xz_filter_device(9, True, dev.data_ptr(), *one, 4)   # SPARC's alignment is 4
        c.xz_filter_device(6, True, dev.data_ptr(), *one, 16)  # IA64's is 16
        c.xz_filter_device(("delta", 256), True, dev.data_ptr(), *one)
        assert (dev.cpu().numpy() == 0).all()


@pytest.mark.kernels_only("one launch of the kernels alone: the configuration does not enter")
def test_the_old_three_are_the_same_kernels(snaphash_mode):
    """x86, ARM and ARM-Thumb through the new entry point give snaphash_bcj_device's bytes (and liblzma's)."""
    import torch
    import bcj_cases as B
    with Context(device=0) as c:
        for filt in B.FILTERS:
            data = B.code(filt, 70000, 9)
            for enc in (True, False):
                dev = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
                torch.cuda.synchronize()
                c.xz_filter_device(B.NAMES[filt], enc, dev.data_ptr(), np.array([0], dtype=np.uint64), np.array([len(data)], dtype=np.uint64), 4096)
                assert c.stats()["launches"] == (2 if filt == B.X86 else 1)
                assert dev.cpu().numpy().tobytes() == B.oracle(filt, enc, data, 4096)
