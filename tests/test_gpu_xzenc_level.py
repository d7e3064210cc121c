"""The .xz producer's level on the GPU: lzma2_chunks_priced_kernel runs xzenc_chunk_priced, the function
the host model runs with a loop for lanes, so its bytes are held against the model's (tests/xzenc_level_host_harness.cpp
through xzenc_level_cases.py) -- the file of snaphash_xz_buffer_ex at level 1 for every input of the CPU tests, and every
array of snaphash_xzenc_stages_device_ex between canaries at launch widths that cut a Block's chunks in two.  Then the
options struct's sizes and refusals, level 1 with a BCJ filter and the self-check, snaphash_tar_create_xz_ex at level 1,
the levels in turn on one context, and the longest launch against the one-second bound."""
import ctypes
import hashlib
import lzma
import os
import subprocess
import tarfile

import numpy as np
import pytest

import trees
import xz_cases as X
import xzenc_cases as E
import xzenc_level_cases as V
from snappy_amd import Context, _lib

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("names FLAG_GPU_ONLY itself")]

CLI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "snappy_amd", "bin", "snaphash")
CANARY = 4096
FILL = 0xA5
ARRAYS = (("prev", np.uint32), ("cand", np.uint32), ("slots", np.uint8), ("res", np.uint32), ("dst", np.uint64), ("out", np.uint8))


@pytest.fixture(scope="module")
def xl():
    return V.load_level()


@pytest.fixture(scope="module")
def kctx(built_lib):
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        yield c


@pytest.fixture(scope="module")
def model(xl):
    """(data, block size, level) -> the model's file: computed once an input and left alone."""
    cache = {}

    def get(data, bs, level=1, filter=0):
        key = (data, bs, level, filter)
        if key not in cache:
            rc, z = V.encode(xl, data, bs, level, filter=filter)
            assert rc == 0
            cache[key] = z
        return cache[key]
    return get


def buffer_ex(c, data, opt):
    """snaphash_xz_buffer_ex itself -> (rc, the file or None)."""
    p, n = ctypes.c_void_p(), ctypes.c_size_t()
    buf = ctypes.create_string_buffer(data, max(len(data), 1))
    rc = _lib.lib().snaphash_xz_buffer_ex(c._h, ctypes.addressof(buf), len(data), ctypes.byref(opt), ctypes.byref(p), ctypes.byref(n))
    if rc:
        assert not p.value and n.value == 0
        return rc, None
    try:
        return 0, ctypes.string_at(p.value, n.value)
    finally:
        _lib.lib().snaphash_free(p)


# ---- 1: the file --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", [n for n, _, _ in V.all_cases()])
def test_level_1_writes_the_host_models_file(kctx, model, name):
    _, data, bs = next(c for c in V.all_cases() if c[0] == name)
    z = kctx.xz_buffer(data, bs, level=1)
    want = model(data, bs)
    assert z == want, "%s: %d bytes, the model %d; first difference at %d" % (
        name, len(z), len(want), next((i for i, (a, b) in enumerate(zip(z, want)) if a != b), min(len(z), len(want))))
    assert lzma.decompress(z) == data


# ---- 2: the stages ------------------------------------------------------------------------------------------------------------


def sizes(n, kw):
    nch = (n + E.CHUNK - 1) // E.CHUNK
    return {"prev": 4 * n, "cand": 4 * n * kw, "slots": nch * V.SLOT, "res": 4 * nch, "dst": 8 * nch, "out": V.out_cap(n)}


def device_stages(c, data, bs, width, level, kw):
    """The entry over `data` in fresh device buffers of FILL; -> the six arrays (canaries checked and cut off) and the
    Blocks' totals.  level None: the plain entry."""
    import torch
    n = len(data)
    sz = sizes(n, kw)
    bufs = {k: torch.full((sz[k] + 2 * CANARY,), FILL, dtype=torch.uint8, device="cuda") for k, _ in ARRAYS}
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    total = c.xzenc_stages_device(d_in.data_ptr(), n, bs, width, *(bufs[k].data_ptr() + CANARY for k, _ in ARRAYS), sz["out"], level=level)
    got = {}
    for k, dt in ARRAYS:
        h = bufs[k].cpu().numpy()
        assert (h[:CANARY] == FILL).all() and (h[CANARY + sz[k]:] == FILL).all(), "the canary around d_%s" % k
        got[k] = h[CANARY:CANARY + sz[k]].copy().view(dt)
    return got, total


def same_arrays(got, total, want, want_total, what):
    for k, _ in ARRAYS:
        if not np.array_equal(got[k], want[k]):
            at = int(np.flatnonzero(got[k] != want[k])[0])
            raise AssertionError("%s: d_%s differs at index %d: %#x, not %#x (%d places in all)"
                                 % (what, k, at, int(got[k][at]), int(want[k][at]), int((got[k] != want[k]).sum())))
    assert total == want_total, what


def test_every_stage_at_level_1_equals_the_model_at_every_launch_width(kctx, xl):
    """Five chunks (the last one short) in Blocks of 256 KiB: width 3 puts the Block's chunks 0 1 2 | 3 4 into two launches,
    width 1 every chunk into its own, 0 is the producer's.  d_cand holds K words a position."""
    data = X.text(2 * E.CHUNK, 301) + V.motifs(2 * E.CHUNK + 4321, 302)
    bs, k = 4 * E.CHUNK, V.consts(xl)[0]
    assert (len(data) + E.CHUNK - 1) // E.CHUNK == 5
    want = V.stages(xl, data, bs, 1, fill=FILL)
    assert want["cand"].size == k * len(data) and (want["cand"].reshape(-1, k)[:, 1] != 0).any()
    for w in (1, 3, 0):
        got, total = device_stages(kctx, data, bs, w, 1, k)
        same_arrays(got, total, want, [int(t) for t in want["total"]], "level 1 at width %d" % w)


def test_level_0_through_the_ex_entry_is_the_plain_entrys_arrays(kctx, xl):
    data = X.text(2 * E.CHUNK + 999, 303)
    plain, plain_total = device_stages(kctx, data, 2 * E.CHUNK, 0, None, 1)
    got, total = device_stages(kctx, data, 2 * E.CHUNK, 0, 0, 1)
    same_arrays(got, total, plain, plain_total, "level 0")
    want = V.stages(xl, data, 2 * E.CHUNK, 0, fill=FILL)
    same_arrays(got, total, want, [int(t) for t in want["total"]], "level 0 against the model")


def test_the_stages_entry_refuses_a_level_it_does_not_have(kctx):
    import torch
    data = X.text(1000, 304)
    sz = sizes(len(data), 4)
    bufs = {k: torch.full((sz[k],), FILL, dtype=torch.uint8, device="cuda") for k, _ in ARRAYS}
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    with pytest.raises(_lib.SnaphashError) as e:
        kctx.xzenc_stages_device(d_in.data_ptr(), len(data), E.CHUNK, 0, *(bufs[k].data_ptr() for k, _ in ARRAYS), sz["out"], level=2)
    assert e.value.code == _lib.EINVAL and "level" in str(e.value)
    assert all(bool((bufs[k] == FILL).all()) for k, _ in ARRAYS)  # nothing was touched


# ---- 3: the struct ------------------------------------------------------------------------------------------------------------


def test_the_options_structs_sizes_and_refusals(kctx, tmp_path):
    data = X.text(70000, 305)
    assert ctypes.sizeof(_lib.XzOptions) == 32 and _lib.XzOptions.level.offset == 24 and _lib.XzOptions.reserved2.offset == 28
    plain = kctx.xz_buffer(data)
    # 24 bytes: the struct every caller before the level was compiled against; whatever lies behind them is not read
    assert buffer_ex(kctx, data, _lib.XzOptions(24, 0, 0, 4, 0, 7, 9)) == (0, plain)
    assert buffer_ex(kctx, data, _lib.XzOptions(32, 0, 0, 4, 0, 0, 0)) == (0, plain)
    assert buffer_ex(kctx, data, _lib.XzOptions(40, 0, 0, 4, 0, 0, 0)) == (0, plain)  # a later, longer struct
    assert buffer_ex(kctx, data, _lib.XzOptions()) == (0, plain)                      # struct_size 0, all zero: the plain entry
    rc, one = buffer_ex(kctx, data, _lib.XzOptions(32, 0, 0, 4, 0, 1, 0))
    assert rc == 0 and one != plain and lzma.decompress(one) == data
    build, _ = trees.make_synthetic_tree(str(tmp_path), [100, 2000])
    out = str(tmp_path / "refused.tar.xz")
    for opt, word in ((_lib.XzOptions(32, 0, 0, 4, 0, 2, 0), "level"), (_lib.XzOptions(32, 0, 0, 4, 0, 0xFFFFFFFF, 0), "level"),
                      (_lib.XzOptions(8, 0, 0, 4, 0, 0, 0), "struct_size"), (_lib.XzOptions(28, 0, 0, 4, 0, 1, 0), "struct_size"),
                      (_lib.XzOptions(32, 0, 0, 4, 0, 0, 1), "reserved2"), (_lib.XzOptions(32, 0, 0, 4, 0, 1, 5), "reserved2")):
        assert buffer_ex(kctx, data, opt) == (_lib.EINVAL, None), word
        why = _lib.lib().snaphash_last_error(kctx._h).decode()
        assert word in why, (word, why)
        y, yl = ctypes.c_void_p(), ctypes.c_size_t()
        assert _lib.lib().snaphash_tar_create_xz_ex(kctx._h, os.fsencode(out), os.fsencode(build), None, ctypes.byref(opt), ctypes.byref(y),
                                                    ctypes.byref(yl), None) == _lib.EINVAL
        assert not y.value and not os.path.exists(out)
    with pytest.raises(_lib.SnaphashError) as e:
        kctx.xz_buffer(data, level=2)
    assert e.value.code == _lib.EINVAL


# ---- 4: with a filter and the self-check ----------------------------------------------------------------------------------------


def test_level_1_with_the_x86_filter_and_the_self_check(kctx, model):
    so = open(os.path.join(os.path.dirname(_lib.__file__), "libsnaphash.so"), "rb").read()
    data = so[:3 * E.CHUNK + 1234] if len(so) > 4 * E.CHUNK else X.text(3 * E.CHUNK + 1234, 306)
    bs = 2 * E.CHUNK
    z = kctx.xz_buffer(data, bs, filter="x86", level=1)
    assert kctx.xz_filter_stats()["filter"] == 4 and kctx.xz_filter_stats()["device_blocks"] == 2
    assert kctx.xz_selfcheck_stats()["chunks"] == 0
    zc = kctx.xz_buffer(data, bs, filter="x86", level=1, self_check=True)
    assert kctx.xz_selfcheck_stats()["chunks"] == kctx.targz_stats()["chunks"] == 4  # every chunk walked and accepted
    assert kctx.xz_filter_stats()["device_blocks"] == 2
    assert zc == z and lzma.decompress(z) == data
    assert z == model(data, bs, 1, 4)
    assert kctx.unxz_buffer(z, bcj=True) == data
    assert len(z) < len(kctx.xz_buffer(data, bs, filter="x86"))


# ---- 5: the tar producer ---------------------------------------------------------------------------------------------------------


def test_tar_create_xz_at_level_1(kctx, tmp_path):
    sizes_ = [0, 1, 100, 511, 512, 513, 4096, 70000, 9999, 31, 20000, 300]  # a dozen files of text: one empty, one over 64 KiB
    build = str(tmp_path / "build")
    for i, n in enumerate(sizes_):
        os.makedirs(os.path.join(build, "d%d" % (i % 3)), exist_ok=True)
        with open(os.path.join(build, "d%d" % (i % 3), "f%02d.txt" % i), "wb") as f:
            f.write(X.text(n, 400 + i))
    a, b = str(tmp_path / "l0.tar.xz"), str(tmp_path / "l1.tar.xz")
    y0, d0 = kctx.tar_create_xz(a, build, with_hashes=True, block_size=E.CHUNK)
    y1, d1 = kctx.tar_create_xz(b, build, with_hashes=True, block_size=E.CHUNK, level=1)
    z0, z1 = open(a, "rb").read(), open(b, "rb").read()
    # hashes.yaml is the level-0 call's but for its first line, which is the archive's own digest
    head0, rest0 = y0.split(b"\n", 1)
    head1, rest1 = y1.split(b"\n", 1)
    assert rest1 == rest0 and rest1
    assert head0 == b"archive-sha512: " + hashlib.sha512(z0).hexdigest().encode() and head1 == b"archive-sha512: " + hashlib.sha512(z1).hexdigest().encode()
    assert d1 == hashlib.sha512(z1).digest() and d0 == hashlib.sha512(z0).digest()
    assert z1 != z0 and lzma.decompress(z1) == lzma.decompress(z0)
    with tarfile.open(b) as tf:
        members = {m.name.lstrip("./"): m for m in tf.getmembers() if m.isfile()}
        assert sorted(m.size for m in members.values()) == sorted(sizes_)
        for name, m in members.items():
            assert tf.extractfile(m).read() == open(os.path.join(build, name), "rb").read(), name
        assert len(members) == len(sizes_)


def test_the_cli_takes_the_level(kctx, model, tmp_path):
    """`snaphash xz -L n` and `snaphash build-xz -L n`: the letter build-bz2 uses for its level."""
    data = X.text(2 * E.CHUNK + 5, 309)
    (tmp_path / "in").write_bytes(data)
    for level in (0, 1):
        out = str(tmp_path / ("l%d.xz" % level))
        subprocess.check_call([CLI, "-g", "xz", str(tmp_path / "in"), out, "-B", "64", "-L", str(level)])
        assert open(out, "rb").read() == model(data, E.CHUNK, level), level
    assert subprocess.run([CLI, "-g", "xz", str(tmp_path / "in"), str(tmp_path / "no.xz"), "-L", "2"], capture_output=True).returncode == 2
    assert not os.path.exists(str(tmp_path / "no.xz"))
    build = str(tmp_path / "build")
    os.makedirs(os.path.join(build, "DEBIAN"))
    for i in range(3):
        with open(os.path.join(build, "f%d.txt" % i), "wb") as f:
            f.write(X.text(30000 + i, 410 + i))
    arcs = []
    for level in (0, 1):
        arc = str(tmp_path / ("l%d.tar.xz" % level))
        out = subprocess.run([CLI, "build-xz", "-L", str(level), build, arc], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        arcs.append(open(arc, "rb").read())
        assert out.stdout.split() == [hashlib.sha512(arcs[-1]).hexdigest(), arc]
    assert lzma.decompress(arcs[1]) == lzma.decompress(arcs[0]) and len(arcs[1]) < len(arcs[0])
    assert subprocess.run([CLI, "build-xz", "-L", "9", build, str(tmp_path / "no.tar.xz")], capture_output=True).returncode == 2


# ---- 6: the levels in turn --------------------------------------------------------------------------------------------------------


def test_the_levels_in_turn_on_one_context_write_what_fresh_contexts_write(kctx, model, built_lib):
    data = X.text(3 * E.CHUNK + 77, 307)
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        first = c.xz_buffer(data, E.CHUNK, level=1)
        zero = c.xz_buffer(data, E.CHUNK, level=0)
        again = c.xz_buffer(data, E.CHUNK, level=1)
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        fresh0 = c.xz_buffer(data, E.CHUNK)
    assert first == again == kctx.xz_buffer(data, E.CHUNK, level=1) == model(data, E.CHUNK, 1)
    assert zero == fresh0 == model(data, E.CHUNK, 0) and zero != first


# ---- 7: the longest launch --------------------------------------------------------------------------------------------------------


def test_the_longest_chunks_launch_stays_under_a_second(kctx, xl):
    """A Block of 1 MiB of motif families in random order (xzenc_level_cases.motifs): most positions have several
    candidates, the windows run full and no match is maximal, so every position is relaxed.  The 16 chunks are one launch.
    deflate_ms is the sum of the call's kernel spans (chains, the chunks launch, concat), so it bounds the launch from above."""
    data = V.motifs(1 << 20, 308)
    kctx.xz_buffer(data[:E.CHUNK], level=1)  # the scratch
    z = kctx.xz_buffer(data, 1 << 20, level=1)
    st = kctx.targz_stats()
    print("level 1, 1 MiB of motifs: kernels %.3f ms for %d chunks, %d bytes out" % (st["deflate_ms"], st["chunks"], len(z)))
    assert st["chunks"] == 16 and st["stored_chunks"] == 0
    assert 0 < st["deflate_ms"] < 1000.0
    assert lzma.decompress(z) == data
