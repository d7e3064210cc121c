"""lzma2_check_kernel alone (snaphash_lzma2_check_device) on the chunk tables of tests/lzma2_check_cases.py: every verdict --
status and offset -- must be the host walker's bit for bit (tests/lzma2_check_host_harness.cpp runs the same header on the
CPU, and tests/test_lzma2_check_host.py holds that walker against liblzma).  Both device buffers lie between 4 KiB of canary
that must come back untouched, and their own bytes are read only.  Tables of 1, 2 and 3 chunks at launch widths 1, 2 and the
producer's, with a refused chunk first, last and alone.  Then the chain: the producer's own kernels
(snaphash_xzenc_stages_device) over every xzenc_cases input and the check over THEIR output in HBM -- every chunk accepted --
and, after one byte of that output is changed from here, exactly that chunk refused."""
import numpy as np
import pytest

import lzma2_check_cases as C
import xzenc_cases as E
from snappy_amd import Context, SnaphashError, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("one kernel on tables the test wrote: names FLAG_GPU_ONLY itself")]

CANARY = 4096
FILL = 0xA5
EINVAL = -1
SLOT = 65600


@pytest.fixture(scope="module")
def L():
    return C.load_harness()


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


def whole(t, data, what):
    h = t.cpu().numpy()
    assert (h[:CANARY] == FILL).all() and (h[CANARY + len(data):] == FILL).all(), "the canary around " + what
    assert bytes(h[CANARY:CANARY + len(data)]) == data, what + " itself was written"


def device_walk(c, d_in, case, d_z, width=0):
    import torch
    torch.cuda.synchronize()
    return c.lzma2_check_device(d_in.data_ptr() + CANARY, len(case.data), case.bs, d_z.data_ptr() + CANARY, len(case.z), case.z_beg, case.z_end,
                                width)


@pytest.mark.parametrize("which", ["good", "damaged"])
def test_case_set_matches_the_host_walker(kctx, L, which):
    cases = C.good_cases(L) if which == "good" else C.damaged_cases(L)
    assert len(cases) > (60 if which == "good" else 150)
    ins = {}
    for c in cases:
        if c.data not in ins:
            ins[c.data] = framed(c.data)
        d_in, d_z = ins[c.data], framed(c.z)
        want = C.host_verdicts(L, c)
        got = device_walk(kctx, d_in, c, d_z)
        assert got == want, "%s: (the kernel's, the host walker's) %s" % (c.name, [x for x in zip(got, want) if x[0] != x[1]][:4])
        if c.expect is not None:
            assert [s for s, _ in got] == c.expect, c.name
        whole(d_z, c.z, "d_z of " + c.name)
        whole(d_in, c.data, "d_in of " + c.name)
    for data, t in ins.items():
        whole(t, data, "d_in")
    assert sum(len(d) for d in ins) < 32 << 20


@pytest.mark.parametrize("nch", [1, 2, 3])
def test_small_tables_at_every_launch_width(kctx, L, nch):
    base = C.model_case(L, "table_%d" % nch, C.X.text((nch - 1) * C.CHUNK + 777, 600 + nch), C.B)
    assert base.nch == nch
    d_in = framed(base.data)
    for width in (1, 2, 0):
        d_z = framed(base.z)
        got = device_walk(kctx, d_in, base, d_z, width)
        assert got == C.host_verdicts(L, base) and [s for s, _ in got] == [C.OK] * nch, width
        for bad in sorted({0, nch - 1}):  # a refused chunk first, last (alone when there is one): its header's size is one off
            z = bytearray(base.z)
            z[base.z_beg[bad] + 2] ^= 1
            c = base.with_("bad_%d" % bad, "header", None, z=bytes(z))
            d_bad = framed(c.z)
            got = device_walk(kctx, d_in, c, d_bad, width)
            assert got == C.host_verdicts(L, c), (width, bad)
            assert [k for k, (s, _) in enumerate(got) if s != C.OK] == [bad] and got[bad][0] == C.USIZE, (width, bad)
            whole(d_bad, c.z, "d_z")
        whole(d_z, base.z, "d_z")
    whole(d_in, base.data, "d_in")


def _chain(c, data, bs):
    """The producer's three kernels over data; -> (d_in, d_out (both framed), the output's bytes, z_beg, z_end, n_z)."""
    import torch
    n = len(data)
    bs_eff = bs or 1 << 20
    nch = (n + C.CHUNK - 1) // C.CHUNK
    cap = n + nch * 64 + 64
    sizes = {"prev": 4 * n, "cand": 4 * n, "slots": nch * SLOT, "res": 4 * nch, "dst": 8 * nch, "out": cap}
    bufs = {k: torch.full((v + 2 * CANARY,), FILL, dtype=torch.uint8, device="cuda") for k, v in sizes.items()}
    d_in = framed(data)
    torch.cuda.synchronize()
    total = c.xzenc_stages_device(d_in.data_ptr() + CANARY, n, bs, 0, *(bufs[k].data_ptr() + CANARY for k in ("prev", "cand", "slots", "res", "dst")),
                                  bufs["out"].data_ptr() + CANARY, cap)
    out = bytes(bufs["out"].cpu().numpy()[CANARY:CANARY + cap])
    z_beg = [int(x) for x in bufs["dst"].cpu().numpy()[CANARY:CANARY + 8 * nch].copy().view(np.uint64)]
    # z_end from the chunk headers the kernels wrote, and each Block's end held against block_total
    cpb, z_end, blk_at = bs_eff // C.CHUNK, [], 0
    for i, b in enumerate(z_beg):
        ctl = out[b]
        size = 3 + (out[b + 1] << 8 | out[b + 2]) + 1 if ctl < 0x80 else 6 + (out[b + 3] << 8 | out[b + 4]) + 1
        last = (i + 1) % cpb == 0 or i + 1 == nch
        z_end.append(b + size + (1 if last else 0))
        if last:
            k = i // cpb
            assert ((z_end[-1] - blk_at + 3) & ~3) + 8 == total[k], "Block %d's end byte is not where block_total puts it" % k
            blk_at += total[k]
    return d_in, bufs["out"], out, z_beg, z_end, sum(total)


@pytest.mark.parametrize("name", [n for n, d, _ in E.cases() if len(d)])
def test_chain_the_producers_output_is_accepted(kctx, L, name):
    import torch
    _, data, bs = E.by_name(name)
    d_in, d_out, out, z_beg, z_end, n_z = _chain(kctx, data, bs)
    case = C.Case("chain_" + name, data, bs or 1 << 20, out[:n_z], z_beg, z_end)
    got = device_walk(kctx, d_in, case, d_out)
    assert got == [(C.OK, min(C.CHUNK, len(data) - i * C.CHUNK)) for i in range(case.nch)], name
    assert got == C.host_verdicts(L, case)
    # one byte of d_out inside one chunk's body, changed from here: exactly that chunk is refused
    bad = case.nch // 2
    hdr = 3 if out[z_beg[bad]] < 0x80 else 6
    last = (bad + 1) % (case.bs // C.CHUNK) == 0 or bad + 1 == case.nch
    body_end = z_end[bad] - (1 if last else 0)  # (the end byte is no part of the body)
    at = z_beg[bad] + hdr + (body_end - z_beg[bad] - hdr) // 2
    assert z_beg[bad] + hdr <= at < body_end
    d_out[CANARY + at] = out[at] ^ 0x10
    torch.cuda.synchronize()
    changed = case.with_("changed", "flip", None, z=out[:at] + bytes([out[at] ^ 0x10]) + out[at + 1:n_z])
    got = device_walk(kctx, d_in, changed, d_out)
    assert got == C.host_verdicts(L, changed), name
    assert [k for k, (s, _) in enumerate(got) if s != C.OK] == [bad], (name, got[bad])
    whole(d_in, data, "d_in")
    h = d_out.cpu().numpy()
    assert (h[:CANARY] == FILL).all() and (h[CANARY + len(out):] == FILL).all(), "the canary around d_out"


def test_refused_arguments(kctx):
    d = framed(b"abc")
    p = d.data_ptr() + CANARY

    def refused(*a):
        with pytest.raises(SnaphashError) as e:
            kctx.lzma2_check_device(*a)
        assert e.value.code == EINVAL

    refused(p, 3, C.B, p, 3, [0], [3], 2049)              # a launch wider than the producer's
    refused(p, 3, C.B, p, 3, [0, 0], [3, 3])              # more chunks than ceil(n_in / 65536)
    refused(p, 65537, C.B, p, 3, [0], [3])                # fewer
    refused(p, 3, 65536 + 512, p, 3, [0], [3])            # a Block size that is no multiple of 64 KiB
    refused(p, 3, 8 << 20, p, 3, [0], [3])                # and one beyond 4 MiB
    refused(0, 3, C.B, p, 3, [0], [3])                    # null staged stream
    refused(p, 3, C.B, 0, 3, [0], [3])                    # null compressed bytes
    refused(p, 0, C.B, p, 3, [], [])                      # no bytes: no chunk
    assert kctx.lzma2_check_device(p, 3, 0, p, 3, [0], [3]) == [(C.BAD, 0)]  # ("abc": 0x61 is no control byte; Block size 0 is 1 MiB)
