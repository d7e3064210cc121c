"""deflate_check_kernel alone (snaphash_deflate_check_device) on the streams of tests/deflate_check_streams.py: every
verdict -- status and offset -- must be the host walker's bit for bit (tests/snapbuild_host_harness.cpp runs the same
header on the CPU, and tests/test_snapbuild_host.py holds that walker against zlib).  Both device buffers lie between
4 KiB of canary that must come back untouched.  Tables of 1, 64 and 257 chunks (a wave, a workgroup round, one more than
the chip's CUs) with a refused chunk first, last and alone among accepted ones."""
import zlib

import numpy as np
import pytest

import deflate_check_streams as S
from snappy_amd import Context, SnaphashError, _lib
from test_snapbuild_host import sb, walk  # noqa: F401  (the host harness, as a fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("one kernel on tables the test wrote: no configuration reaches it")]

CANARY = 4096
FILL = 0xA5
EINVAL = -1


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


def framed(data):
    """bytes -> a device tensor: canary, the bytes, canary"""
    import torch
    h = np.full(len(data) + 2 * CANARY, FILL, dtype=np.uint8)
    h[CANARY:CANARY + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return torch.from_numpy(h).cuda()


def canaries_whole(t, n, what):
    h = t.cpu().numpy()
    assert (h[:CANARY] == FILL).all() and (h[CANARY + n:] == FILL).all(), "the canary around " + what


def device_walk(c, d_in, n_in, d_z, z_off, final):
    import torch
    torch.cuda.synchronize()
    return c.deflate_check_device(d_in.data_ptr() + CANARY, n_in, d_z.data_ptr() + CANARY, z_off, final)


def test_stream_set_matches_the_host_walker(kctx, sb):
    cases = S.all_cases()
    assert len(cases) > 190
    ins, total = {}, 0
    for name, data, z, z_off, final, good in cases:
        if data not in ins:
            ins[data] = framed(data)
            total += len(data)
        d_in, d_z = ins[data], framed(z)
        want = walk(sb, data, z, z_off, final)
        got = device_walk(kctx, d_in, len(data), d_z, z_off, final)
        assert got == want, "%s: the kernel %s, the host walker %s" % (name, got, want)
        if good:
            assert [s for s, _ in got] == [S.OK] * len(got), name
        canaries_whole(d_z, len(z), "d_z of " + name)
        # the staged bytes and the compressed bytes themselves are read only
        assert bytes(d_z.cpu().numpy()[CANARY:CANARY + len(z)]) == z
    for data, t in ins.items():
        canaries_whole(t, len(data), "d_in")
        assert bytes(t.cpu().numpy()[CANARY:CANARY + len(data)]) == data
    assert total < 20 << 20


def big_table(nch, last_len):
    """nch chunks of text (the last one last_len bytes), zlib level 1 with a flush a chunk"""
    base = S.payload(300000, 21)
    n = (nch - 1) * S.CHUNK + last_len
    data = (base * (n // len(base) + 1))[:n]
    z, off = S.zlib_stream(data, 1, False)
    assert len(off) - 1 == nch
    return data, z, off


@pytest.mark.parametrize("nch,last_len", [(1, 1000), (64, 1), (257, 1)])
def test_table_sizes_with_one_refused_chunk(kctx, sb, nch, last_len):
    import torch
    data, z, off = big_table(nch, last_len)
    assert len(data) < 17 << 20
    d_in, d_z = framed(data), framed(z)
    got = device_walk(kctx, d_in, len(data), d_z, off, False)
    assert got == walk(sb, data, z, off, False)
    assert [s for s, _ in got] == [S.OK] * nch
    for bad in sorted({0, nch // 2, nch - 1}):
        at = bad * S.CHUNK + (0 if bad == nch - 1 else 12345)  # a staged byte of that chunk alone...
        changed = bytearray(data)
        changed[at] ^= 0x40
        d_in[CANARY + at] = changed[at]
        got = device_walk(kctx, d_in, len(data), d_z, off, False)
        want = walk(sb, bytes(changed), z, off, False)
        assert got == want, "refused chunk %d of %d" % (bad, nch)
        # ... is refused where it differs; zlib's window lets later chunks copy from it, so those may be refused too
        assert got[bad][0] in (S.LITERAL, S.MATCH) and got[bad][1] <= at - bad * S.CHUNK
        assert [s for s, _ in got[:bad]] == [S.OK] * bad
        d_in[CANARY + at] = data[at]
    # a refused chunk ALONE among accepted ones: damage only its own stretch's last block header (LEN of the empty stored block)
    for bad in sorted({0, nch // 2, nch - 1}):
        zz = bytearray(z)
        zz[off[bad + 1] - 4] ^= 0x01
        d_bad = framed(bytes(zz))
        got = device_walk(kctx, d_in, len(data), d_bad, off, False)
        assert got == walk(sb, data, bytes(zz), off, False)
        assert [k for k, (s, _) in enumerate(got) if s != S.OK] == [bad]
        canaries_whole(d_bad, len(z), "d_z")
    canaries_whole(d_in, len(data), "d_in")
    canaries_whole(d_z, len(z), "d_z")
    torch.cuda.synchronize()


def test_final_block_on_the_last_chunk(kctx, sb):
    data = S.payload(2 * S.CHUNK + 77, 5)
    z, off = S.zlib_stream(data, 9, True)
    assert zlib.decompress(z, -15) == data
    d_in, d_z = framed(data), framed(z)
    got = device_walk(kctx, d_in, len(data), d_z, off, True)
    assert got == walk(sb, data, z, off, True) and [s for s, _ in got] == [S.OK] * 3
    got = device_walk(kctx, d_in, len(data), d_z, off, False)  # BFINAL where none may be
    assert got == walk(sb, data, z, off, False) and [s for s, _ in got] == [S.OK, S.OK, S.BAD]


def test_refused_arguments(kctx):
    d = framed(b"abc")
    p = d.data_ptr() + CANARY

    def refused(*a):
        with pytest.raises(SnaphashError) as e:
            kctx.deflate_check_device(*a)
        assert e.value.code == EINVAL

    refused(p, 3, p, [0])                  # no chunk
    refused(p, 65537, p, [0, 3])           # too few chunks for the bytes
    refused(p, 3, p, [0, 3, 2])            # offsets that descend
    refused(0, 3, p, [0, 3])               # null staged stream
    refused(p, 3, 0, [0, 3])               # null compressed bytes
    assert kctx.deflate_check_device(0, 0, 0, [0, 0]) == [(S.OK, 0)]
