#!/usr/bin/env python3
"""data.tar.bz2 measured: the GPU bzip2 decode and the default configuration against the reference's shape (Go's
compress/bzip2: one block after another on one core; Python's bz2, libbz2, on one core stands in for it).

  buffer     snaphash_bunzip2_buffer on tools/deflate_corpora.py's text, sources and binaries (64 MiB each) at levels 1
             and 9: the GPU-only call (its decode kernels' time from HIP events, output GB/s over kernel time and over the
             call) and the default call, beside bz2.decompress on one core
  unpack     tar_unpack_bz2 with hashes.yaml on a package the shape of tools/unpack_bench.py's (297 files, 256 MiB) in
             both configurations, beside tarfile's extraction + snaphash_verify (two reads)
The split of the kernel time over the stages (scan, symbols, inverse BWT, RLE1) comes from a run of this script under
`rocprofv3 --kernel-trace --stats` (profiles/r07_bunzip2_kernel_stats.csv).
usage: tools/bunzip2_bench.py [--quick] [--out FILE]    (JSON lines on stdout and in FILE)"""
import argparse
import bz2
import io
import json
import os
import shutil
import sys
import tarfile
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from snappy_amd import Context, _lib  # noqa: E402
from unpack_bench import best, corpora, emit  # noqa: E402


def package(root, total, files, seed):
    """`files` files of mixed text and binary content, `total` bytes in all, under root/build."""
    rng = np.random.default_rng(seed)
    c = corpora(8 << 20)
    pool = [c["text"], c["sources"], c["binaries"]]
    build = os.path.join(root, "build")
    os.makedirs(os.path.join(build, "DEBIAN"))
    sizes = rng.pareto(1.2, size=files) + 1
    sizes = (sizes / sizes.sum() * total).astype(np.int64)
    for i, n in enumerate(sizes):
        d = os.path.join(build, "d%02d" % (i % 17))
        os.makedirs(d, exist_ok=True)
        src = pool[i % 3]
        off = int(rng.integers(0, len(src)))
        data = (src[off:] + src)[: int(n)] if n <= len(src) else (src * (int(n) // len(src) + 1))[: int(n)]
        with open(os.path.join(d, "f%04d" % i), "wb") as f:
            f.write(data)
    return build


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    size = (8 << 20) if a.quick else (64 << 20)
    reps = 1 if a.quick else 3
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
        for name, data in corpora(size).items():
            for lv in (1, 9):
                z = bz2.compress(data, lv)
                t_gpu, out = best(lambda: g.bunzip2_buffer(z), reps)
                assert out == data
                sg = g.unpack_stats()
                t_def, out = best(lambda: d.bunzip2_buffer(z), reps)
                assert out == data
                t_one, out = best(lambda: bz2.decompress(z), 1 if a.quick else 2)
                emit({"leg": "buffer", "corpus": name, "level": lv, "bytes": len(data), "bz2_bytes": len(z), "blocks": sg["segments"],
                      "gpu_blocks": sg["gpu_segments"], "kernel_ms": round(sg["inflate_ms"], 2),
                      "kernel_gbps": round(len(data) / sg["inflate_ms"] / 1e6, 3) if sg["inflate_ms"] else None,
                      "gpu_only_ms": round(t_gpu * 1e3, 2), "gpu_only_gbps": round(len(data) / t_gpu / 1e9, 3),
                      "default_ms": round(t_def * 1e3, 2), "default_gbps": round(len(data) / t_def / 1e9, 3),
                      "libbz2_one_core_ms": round(t_one * 1e3, 2), "libbz2_one_core_gbps": round(len(data) / t_one / 1e9, 3),
                      "gpu_only_vs_one_core": round(t_one / t_gpu, 2), "default_vs_one_core": round(t_one / t_def, 2)}, fh)
        tmp = tempfile.mkdtemp(prefix="bz2bench")
        try:
            total = (32 << 20) if a.quick else (256 << 20)
            build = package(tmp, total, 297, 5)
            arc_gz = os.path.join(tmp, "data.tar.gz")
            yaml, _ = d.tar_create(arc_gz, build, build + "/DEBIAN", with_hashes=True)
            import gzip
            import hashlib
            arc = os.path.join(tmp, "data.tar.bz2")
            with open(arc, "wb") as f:
                f.write(bz2.compress(gzip.decompress(open(arc_gz, "rb").read()), 9))
            dig = hashlib.sha512(open(arc, "rb").read()).hexdigest().encode()
            yaml = b"\n".join(b"archive-sha512: " + dig if ln.startswith(b"archive-sha512: ") else ln for ln in yaml.split(b"\n"))
            rec = {"leg": "unpack", "files": 297, "bytes": total, "bz2_bytes": os.path.getsize(arc)}
            for label, ctx in (("gpu_only", g), ("default", d)):
                ts = []
                for r in range(reps):
                    tgt = os.path.join(tmp, "u_%s_%d" % (label, r))
                    t0 = time.perf_counter()
                    mis, _ = ctx.tar_unpack_bz2(arc, tgt, yaml)
                    ts.append(time.perf_counter() - t0)
                    assert mis is None, mis
                    shutil.rmtree(tgt)
                rec[label + "_ms"] = round(min(ts) * 1e3, 2)
                rec[label + "_kernel_ms"] = round(ctx.unpack_stats()["inflate_ms"], 2)
            t0 = time.perf_counter()
            tgt = os.path.join(tmp, "ref")
            with tarfile.open(arc, "r:bz2") as t:
                t.extractall(tgt)
            mis = d.verify(tgt, yaml, arc)
            rec["tarfile_plus_verify_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
            assert mis is None, mis
            rec["default_vs_two_reads"] = round(rec["tarfile_plus_verify_ms"] / rec["default_ms"], 2)
            rec["gpu_only_vs_two_reads"] = round(rec["tarfile_plus_verify_ms"] / rec["gpu_only_ms"], 2)
            emit(rec, fh)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
