#!/usr/bin/env python3
"""data.tar.xz measured: the GPU LZMA2 decode and the default configuration against the reference's shape (the xz program:
one Block after another on one core; Python's lzma, liblzma, on one core stands in for it).

  buffer     snaphash_unxz_buffer on tools/deflate_corpora.py's text, sources and binaries (64 MiB each), each compressed
             by Python's lzma in two shapes -- one Block (what `xz --compress --stdout` writes) and Blocks of 1 MiB
             assembled by tests/xz_cases.py's xz_file (what `xz -T` / `--block-size` write): the GPU-only call (its decode
             and Check kernels' time from HIP events, output GB/s over kernel time and over the call, the Blocks the
             kernel took and the bytes that went to host threads because a Block was over kXzGpuBlockMax), the default
             call, and lzma.decompress on one core; best of --reps with the worst beside it
  crc64      snaphash_crc64_device on 64 MiB of random bytes in HBM, as one range and as 1 024 ranges: kernel time (HIP
             events), GB/s over it, the fraction of the 8 TB/s HBM peak (the kernel reads every byte once), the call's
             wall time
  unpack     tar_unpack_xz with hashes.yaml on a package the shape of tools/unpack_bench.py's (297 files, 256 MiB; Blocks
             of 1 MiB) in both configurations, beside tarfile's extraction + snaphash_verify (two reads)
The longest single launch is what kXzGpuBlockMax (xz_kernels.h) is set by: the `kernel_ms` of the 1 MiB-Block rows is one
launch each.
usage: tools/unxz_bench.py [--quick] [--reps N] [--preset P] [--legs buffer,crc64,unpack] [--out FILE]
(JSON lines on stdout and in FILE)"""
import argparse
import gzip
import hashlib
import lzma
import os
import shutil
import sys
import tarfile
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from snappy_amd import Context, _lib  # noqa: E402
from bunzip2_bench import package  # noqa: E402
from unpack_bench import HBM_PEAK, corpora, emit  # noqa: E402
import xz_cases  # noqa: E402

BLOCK = 1 << 20


def timed(fn, reps):
    """-> (best seconds, worst seconds, the last result)"""
    t, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return min(t), max(t), out


def blocks_xz(data, preset):
    """`data` as one Stream of 1 MiB Blocks with CRC-64 Checks (the Blocks compressed side by side: liblzma drops the GIL)."""
    def one(i):
        piece = data[i:i + BLOCK]
        f = dict(id=lzma.FILTER_LZMA2, preset=preset, dict_size=BLOCK)  # a Block never reaches further back than itself
        return lzma.compress(piece, format=lzma.FORMAT_RAW, filters=[f]), piece, BLOCK
    with ThreadPoolExecutor(16) as ex:
        blocks = list(ex.map(one, range(0, len(data), BLOCK)))
    return xz_cases.xz_file(blocks, xz_cases.CHECK_CRC64)


def buffer_leg(g, d, size, reps, preset, fh):
    for name, data in corpora(size).items():
        for shape, z in (("one_block", lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=preset)),
                         ("blocks_1mib", blocks_xz(data, preset))):
            g.unxz_buffer(z)  # warm: the scratch
            ks = []

            def gpu_call():
                out = g.unxz_buffer(z)
                ks.append(g.unpack_stats()["inflate_ms"])
                return out
            t_gpu, t_gpu_max, out = timed(gpu_call, reps)
            assert out == data
            sg = g.unpack_stats()
            t_def, t_def_max, out = timed(lambda: d.unxz_buffer(z), reps)
            assert out == data
            t_one, t_one_max, out = timed(lambda: lzma.decompress(z), max(1, reps - 1))
            assert out == data
            k = min(ks)
            emit({"leg": "buffer", "corpus": name, "shape": shape, "preset": preset, "bytes": len(data), "xz_bytes": len(z),
                  "blocks": sg["segments"], "gpu_blocks": sg["gpu_segments"], "gpu_only_host_bytes": sg["host_bytes"],
                  "kernel_ms": round(k, 2), "kernel_ms_max": round(max(ks), 2),
                  "kernel_gbps": round((len(data) - sg["host_bytes"]) / k / 1e6, 3) if k else None,
                  "gpu_only_ms": round(t_gpu * 1e3, 2), "gpu_only_ms_max": round(t_gpu_max * 1e3, 2),
                  "gpu_only_gbps": round(len(data) / t_gpu / 1e9, 3),
                  "default_ms": round(t_def * 1e3, 2), "default_ms_max": round(t_def_max * 1e3, 2),
                  "default_gbps": round(len(data) / t_def / 1e9, 3),
                  "liblzma_one_core_ms": round(t_one * 1e3, 2), "liblzma_one_core_ms_max": round(t_one_max * 1e3, 2),
                  "liblzma_one_core_gbps": round(len(data) / t_one / 1e9, 3),
                  "gpu_only_vs_one_core": round(t_one / t_gpu, 2), "default_vs_one_core": round(t_one / t_def, 2)}, fh)


def crc64_leg(g, size, reps, fh):
    import torch
    host = np.random.default_rng(1).integers(0, 256, size, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    want = xz_cases.crc64_fast(host[:1 << 20].tobytes())
    assert int(g.crc64_device(dev.data_ptr(), np.zeros(1, dtype=np.uint64), np.full(1, 1 << 20, dtype=np.uint64))[0]) == want
    for nr in (1, 1024):
        step = size // nr
        offs = np.arange(nr, dtype=np.uint64) * np.uint64(step)
        lens = np.full(nr, step, dtype=np.uint64)
        g.crc64_device(dev.data_ptr(), offs, lens)  # warm: the scratch
        ks, ws = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.crc64_device(dev.data_ptr(), offs, lens)
            ws.append(time.perf_counter() - t0)
            ks.append(g.stats()["kernel_ms"])
        k = min(ks)
        emit({"leg": "crc64", "ranges": nr, "bytes": size, "kernel_ms": round(k, 4), "kernel_ms_max": round(max(ks), 4),
              "kernel_gbps": round(size / k / 1e6, 1), "hbm_fraction": round(size / (k / 1e3) / HBM_PEAK, 4),
              "call_ms": round(min(ws) * 1e3, 3), "call_ms_max": round(max(ws) * 1e3, 3)}, fh)


def unpack_leg(g, d, total, reps, preset, fh):
    tmp = tempfile.mkdtemp(prefix="xzbench")
    try:
        build = package(tmp, total, 297, 5)
        arc_gz = os.path.join(tmp, "data.tar.gz")
        yaml, _ = d.tar_create(arc_gz, build, build + "/DEBIAN", with_hashes=True)
        arc = os.path.join(tmp, "data.tar.xz")
        with open(arc, "wb") as f:
            f.write(blocks_xz(gzip.decompress(open(arc_gz, "rb").read()), preset))
        dig = hashlib.sha512(open(arc, "rb").read()).hexdigest().encode()
        yaml = b"\n".join(b"archive-sha512: " + dig if ln.startswith(b"archive-sha512: ") else ln for ln in yaml.split(b"\n"))
        rec = {"leg": "unpack", "files": 297, "bytes": total, "xz_bytes": os.path.getsize(arc), "preset": preset}
        for label, ctx in (("gpu_only", g), ("default", d)):
            ts = []
            for r in range(reps):
                tgt = os.path.join(tmp, "u_%s_%d" % (label, r))
                t0 = time.perf_counter()
                mis, _ = ctx.tar_unpack_xz(arc, tgt, yaml)
                ts.append(time.perf_counter() - t0)
                assert mis is None, mis
                shutil.rmtree(tgt)
            rec[label + "_ms"] = round(min(ts) * 1e3, 2)
            rec[label + "_ms_max"] = round(max(ts) * 1e3, 2)
            rec[label + "_kernel_ms"] = round(ctx.unpack_stats()["inflate_ms"], 2)
        t0 = time.perf_counter()
        tgt = os.path.join(tmp, "ref")
        with tarfile.open(arc, "r:xz") as t:
            t.extractall(tgt)
        mis = d.verify(tgt, yaml, arc)
        rec["tarfile_plus_verify_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
        assert mis is None, mis
        rec["default_vs_two_reads"] = round(rec["tarfile_plus_verify_ms"] / rec["default_ms"], 2)
        rec["gpu_only_vs_two_reads"] = round(rec["tarfile_plus_verify_ms"] / rec["gpu_only_ms"], 2)
        emit(rec, fh)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--preset", type=int, default=6)
    ap.add_argument("--legs", default="buffer,crc64,unpack")
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    legs = a.legs.split(",")
    size = (8 << 20) if a.quick else (64 << 20)
    reps = 1 if a.quick else a.reps
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
        if "crc64" in legs:
            crc64_leg(g, size, max(reps, 3), fh)
        if "buffer" in legs:
            buffer_leg(g, d, size, reps, a.preset, fh)
        if "unpack" in legs:
            unpack_leg(g, d, (32 << 20) if a.quick else (256 << 20), reps, a.preset, fh)


if __name__ == "__main__":
    main()
