"""Which timing fields every entry fills, call after call: one fresh Context, each entry twice in a row on the smallest
input that makes it launch.  The engine times its launches with HIP events that it keeps between calls; a pair read
twice, or not cleared where a call ends, shows here as a field that turns positive, or as a second call that reports the
first one's time with its own.  The table below is what the library reported before its events and streams got owners
(snappy_amd/csrc/gpu_handles.h), so the module passes unchanged on either side of that change.

After each call: the fields listed as positive are positive and the others zero, both times; `launches` is the same both
times; and no field of the second call exceeds the first call's plus the second call's wall time.  Two children check
that the stage lines of SNAPHASH_TRACE_BZ2 and SNAPHASH_TRACE_XZ still match the patterns the bench tools read."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("names its own flags: every byte through the kernels")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB64 = 64 << 10

# entry -> the timing fields that are positive after it; every other field of FIELDS is zero.  (Fields of another
# entry's stats -- the self-checks', the filter's, the unpack's -- keep what the last call of their kind left: the
# order of ENTRIES is part of the table.)
FIELDS = ("kernel_ms", "h2d_ms", "launches", "deflate_ms", "xz_selfcheck_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms")
POSITIVE = {
    "sha512_buffers": ("kernel_ms", "h2d_ms", "launches"),
    "gzip_buffer": ("h2d_ms", "deflate_ms"),
    "xz_buffer": ("h2d_ms", "deflate_ms"),
    "xz_buffer_self_check": ("h2d_ms", "deflate_ms", "xz_selfcheck_ms"),
    "xz_buffer_x86": ("h2d_ms", "deflate_ms", "filter_device_ms"),
    "bzip2_buffer": ("h2d_ms", "deflate_ms", "filter_device_ms"),  # (the filter's stats are the last .xz call's)
    "bzip2_buffer_self_check": ("h2d_ms", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms"),
    "gunzip_buffer": ("deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "bunzip2_buffer": ("deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "unxz_buffer": ("deflate_ms", "bz2_selfcheck_ms", "inflate_ms"),  # (an .xz call without a filter: its stats say none ran)
    "unxz_buffer_x86": ("deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "crc32_device": ("kernel_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "crc64_device": ("kernel_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "sha256_device": ("kernel_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "bcj_device": ("kernel_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "files_equal": ("kernel_ms", "h2d_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
    "tar_create": ("kernel_ms", "h2d_ms", "launches", "deflate_ms", "bz2_selfcheck_ms", "filter_device_ms", "inflate_ms"),
}


def text(n, seed=7):
    """n bytes that compress: words of a small vocabulary, seeded."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, int(k), dtype=np.uint8)) for k in rng.integers(2, 10, 300)]
    out = b" ".join(words[i] for i in rng.integers(0, len(words), n // 3))
    return out[:n].ljust(n, b".")


def figures(c, wall):
    s, u = c.stats(), c.unpack_stats()
    return {"kernel_ms": s["kernel_ms"], "h2d_ms": s["h2d_ms"], "launches": s["launches"], "deflate_ms": c.targz_stats()["deflate_ms"],
            "xz_selfcheck_ms": c.xz_selfcheck_stats()["ms"], "bz2_selfcheck_ms": c.bz2_selfcheck_stats()["ms"],
            "filter_device_ms": c.xz_filter_stats()["device_ms"], "inflate_ms": u["inflate_ms"],
            "wall_ms": s["wall_ms"] if s["wall_ms"] > 0 else wall}


@pytest.fixture(scope="module")
def runs(built_lib, tmp_path_factory):
    """{entry: (figures after the first call, after the second)}, every entry of the table in order on one Context."""
    import torch
    from snappy_amd import Context, _lib
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    data = text(KIB64)
    dev = torch.from_numpy(np.frombuffer(text(4096, seed=8), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    one = (np.zeros(1, dtype=np.uint64), np.full(1, 4096, dtype=np.uint64))
    tmp = tmp_path_factory.mktemp("timing")
    pairs = []
    for k in range(2):
        a, b = tmp / ("a%d" % k), tmp / ("b%d" % k)
        a.write_bytes(text(4096, seed=20 + k))
        b.write_bytes(text(4096, seed=20 + k))
        pairs.append((str(a), str(b)))
    tree = tmp / "tree"
    tree.mkdir()
    for name, n in (("one", 1), ("two", 111), ("three", 129), ("empty", 0)):
        (tree / name).write_bytes(text(n, seed=30 + n))
    made = {}
    out = {}
    print("timing fields: library %s" % _lib.LIB_PATH)
    with Context(flags=_lib.FLAG_GPU_ONLY) as c:
        entries = [
            ("sha512_buffers", lambda: c.sha512_buffers([text(1), text(111), text(129)])),
            ("gzip_buffer", lambda: made.__setitem__("gz", c.gzip_buffer(data))),
            ("xz_buffer", lambda: made.__setitem__("xz", c.xz_buffer(data))),
            ("xz_buffer_self_check", lambda: c.xz_buffer(data, self_check=True)),
            ("xz_buffer_x86", lambda: made.__setitem__("xz_x86", c.xz_buffer(data, filter="x86"))),
            ("bzip2_buffer", lambda: made.__setitem__("bz2", c.bzip2_buffer(data, level=1))),
            ("bzip2_buffer_self_check", lambda: c.bzip2_buffer(data, level=1, self_check=True)),
            ("gunzip_buffer", lambda: made.__setitem__("gunzip", c.gunzip_buffer(made["gz"]))),
            ("bunzip2_buffer", lambda: made.__setitem__("bunzip2", c.bunzip2_buffer(made["bz2"]))),
            ("unxz_buffer", lambda: made.__setitem__("unxz", c.unxz_buffer(made["xz"]))),
            ("unxz_buffer_x86", lambda: made.__setitem__("unxz_x86", c.unxz_buffer(made["xz_x86"], bcj=True))),
            ("crc32_device", lambda: c.crc32_device(_lib.CRC_GZIP, dev.data_ptr(), *one)),
            ("crc64_device", lambda: c.crc64_device(dev.data_ptr(), *one)),
            ("sha256_device", lambda: c.sha256_device(dev.data_ptr(), *one)),
            ("bcj_device", lambda: c.bcj_device("x86", True, dev.data_ptr(), *one)),
            ("files_equal", lambda: made.__setitem__("equal", c.files_equal(pairs))),
            ("tar_create", lambda: c.tar_create(str(tmp / "data.tar.gz"), str(tree), with_hashes=True)),
        ]
        assert [e for e, _ in entries] == list(ENTRIES)
        for name, call in entries:
            both = []
            for _ in range(2):
                t0 = time.perf_counter()
                call()
                both.append(figures(c, (time.perf_counter() - t0) * 1e3))
            print("timing fields: %-24s first %s" % (name, {k: round(v, 4) for k, v in both[0].items()}))
            print("timing fields: %-24s second %s" % (name, {k: round(v, 4) for k, v in both[1].items()}))
            out[name] = tuple(both)
    # (the calls did what they were made for: the table is about launches that ran)
    assert made["gunzip"] == data and made["bunzip2"] == data and made["unxz"] == data and made["unxz_x86"] == data and made["equal"] == [True, True]
    return out


ENTRIES = ("sha512_buffers", "gzip_buffer", "xz_buffer", "xz_buffer_self_check", "xz_buffer_x86", "bzip2_buffer", "bzip2_buffer_self_check",
           "gunzip_buffer", "bunzip2_buffer", "unxz_buffer", "unxz_buffer_x86", "crc32_device", "crc64_device", "sha256_device", "bcj_device",
           "files_equal", "tar_create")


@pytest.mark.parametrize("entry", ENTRIES)
def test_fields_are_the_same_call_after_call(runs, entry):
    first, second = runs[entry]
    for got in (first, second):
        assert {f for f in FIELDS if got[f] > 0} == set(POSITIVE[entry]), (entry, got)
        assert all(got[f] >= 0 for f in FIELDS), (entry, got)
    assert first["launches"] == second["launches"], (entry, first, second)
    # a second call that reports the first one's time with its own (a ledger not cleared where the first ended)
    for f in FIELDS:
        if f != "launches":
            assert second[f] <= first[f] + second["wall_ms"], (entry, f, first, second)


CHILD = """
import sys
sys.path.insert(0, %r)
from snappy_amd import Context, _lib
data = open(sys.argv[2], "rb").read()
with Context(flags=_lib.FLAG_GPU_ONLY) as c:
    z = c.bzip2_buffer(data, level=1) if sys.argv[1] == "bz2" else c.xz_buffer(data)
print(len(z))
"""


@pytest.mark.parametrize("which, env", [("bz2", "SNAPHASH_TRACE_BZ2"), ("xz", "SNAPHASH_TRACE_XZ")])
def test_trace_lines_match_the_bench_tools_patterns(built_lib, tmp_path, which, env):
    """The stage line of a 64 KiB call, in a fresh child with the trace on, against the pattern its bench tool reads."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import bzip2_enc_bench
        import xz_bench
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    pattern = bzip2_enc_bench.TRACE if which == "bz2" else xz_bench.TRACE
    src = tmp_path / "in"
    src.write_bytes(text(KIB64))
    r = subprocess.run([sys.executable, "-c", CHILD % ROOT, which, str(src)], env=dict(os.environ, **{env: "1"}), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stderr.splitlines() if ln.startswith("snaphash %s: slot of " % which)]
    assert len(lines) == 1 and pattern.search(lines[0]), r.stderr[-4000:]
    assert all(float(g) >= 0 for g in pattern.search(lines[0]).groups()), lines[0]
