#!/usr/bin/env python3
"""Row f5 measured: the GPU inflate and the install-side unpack + Verify against the reference's shape.

  kernel     snaphash_gunzip_buffer in the GPU-only configuration on tools/deflate_corpora.py's text, sources and binaries
             (64 MiB each, compressed by the library's own producer): inflate kernel time (scan + decode + fill + concat,
             HIP events), output GB/s over kernel time and over the call, and the kernel's HBM traffic as a fraction of
             the 8 TB/s peak (it reads the stream and writes two bytes a symbol into its slots, then one byte out)
  gunzip     gunzip_buffer end to end, both configurations, beside Python's zlib on one core (the reference's shape:
             one inflate on one core)
  unpack     tar_unpack with hashes.yaml on a package the size of config 2 (a tree of ~250 MiB) and on 1 GiB of text,
             beside two baselines: Python zlib + tarfile + snaphash_verify (two reads), and zlib on one core alone
  plain      streams WITHOUT flush points (Python zlib -9, as click build / dpkg-deb / Go's gzip.Writer write them):
             gunzip without SNAPHASH_FLAG_SPLIT_BLOCKS (the serial route), with it in both configurations, and zlib on
             one core; the block scan's time per 64 MiB and its unreached (false) candidates per MiB; then tar_unpack
             with Verify of a config-2-sized package written by tarfile in "w:gz" mode (zlib -9), with and without the flag
usage: tools/unpack_bench.py [--quick] [--legs kernel,unpack,plain] [--out FILE]    (JSON lines on stdout and in FILE)"""
import argparse
import io
import json
import os
import shutil
import sys
import tarfile
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from snappy_amd import Context, _lib  # noqa: E402

HBM_PEAK = 8.0e12


def corpora(size):
    import importlib.util
    spec = importlib.util.spec_from_file_location("deflate_corpora_src", os.path.join(ROOT, "tools", "deflate_corpora.py"))
    src = open(spec.origin).read().split("depths = ")[0]  # the corpus builders, not the script's own run
    g = {"__name__": "deflate_corpora_src", "__file__": spec.origin}
    exec(compile(src, spec.origin, "exec"), g)
    g["SIZE"] = size
    return {"text": g["text"](), "sources": g["fill"](g["sources"]()), "binaries": g["fill"](g["binaries"]())}


def best(fn, reps):
    t = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return min(t), out


def emit(rec, fh):
    line = json.dumps(rec)
    print(line, flush=True)
    if fh:
        fh.write(line + "\n")
        fh.flush()


def make_package(root, total, seed):
    """A tree of files like config 2 (sizes from 1 KiB to 8 MiB, text and binary), `total` bytes."""
    rng = np.random.default_rng(seed)
    words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 10)), dtype=np.uint8)) for _ in range(2000)]
    os.makedirs(root)
    n, k = 0, 0
    while n < total:
        sz = int(min(total - n, 2 ** rng.uniform(10, 23)))
        if k % 3 == 2:
            data = rng.integers(0, 256, size=sz, dtype=np.uint8).tobytes()
        else:
            data = b" ".join(words[int(i)] for i in rng.zipf(1.3, size=sz // 5 + 8) % 2000)[:sz]
        d = os.path.join(root, "d%02d" % (k % 37))
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "f%05d" % k), "wb") as f:
            f.write(data)
        n += sz
        k += 1
    return k


def _gz9(data):
    c = zlib.compressobj(9, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def plain(size, reps, pkg_total, fh):
    """The plain leg: no flush points, so without the flag every byte is the serial host decoder's."""
    G, S = _lib.FLAG_GPU_ONLY, _lib.FLAG_SPLIT_BLOCKS
    with Context(device=0, flags=0) as d, Context(device=0, flags=S) as ds, Context(device=0, flags=G | S) as gs:
        for name, data in corpora(size).items():
            gz = _gz9(data)
            row = {"leg": "plain", "corpus": name, "bytes": len(data), "gz_bytes": len(gz)}
            z1, zout = best(lambda: zlib.decompress(gz, 31), reps)
            assert zout == data
            row["zlib_one_core_ms"] = round(z1 * 1e3, 2)
            for cname, ctx in (("serial", d), ("split_default", ds), ("split_gpu_only", gs)):
                ctx.gunzip_buffer(gz)  # warm: the scratch buffers
                t, out = best(lambda: ctx.gunzip_buffer(gz), reps)
                assert out == data
                st, bs = ctx.unpack_stats(), ctx.block_scan_stats()
                row[cname + "_ms"] = round(t * 1e3, 2)
                row[cname + "_segments"] = [st["gpu_segments"], st["segments"]]
                row[cname + "_host_bytes"] = st["host_bytes"]
                if ctx is not d:
                    row[cname + "_vs_serial"] = round(row["serial_ms"] / row[cname + "_ms"], 2)
                    row[cname + "_vs_one_core"] = round(z1 / t, 2)
                    mib = bs["bits_scanned"] / 8 / (1 << 20)
                    row[cname + "_scan"] = {"scan_ms": round(bs["scan_ms"], 3), "scan_ms_per_64MiB": round(bs["scan_ms"] / mib * 64, 3),
                                            "candidates": bs["candidates"], "linked": bs["linked"], "unreached": bs["unreached"],
                                            "unreached_per_MiB": round(bs["unreached"] / mib, 3), "host_blocks": bs["host_blocks"]}
            emit(row, fh)
        # near the block route's threshold (a member that starts with 1 MiB of the stream left): small text streams
        text = corpora(size)["text"]
        for mib in (4, 8, 16):
            data = text[: mib << 20]
            gz = _gz9(data)
            row = {"leg": "plain_small", "bytes": len(data), "gz_bytes": len(gz)}
            z1, _ = best(lambda: zlib.decompress(gz, 31), reps)
            row["zlib_one_core_ms"] = round(z1 * 1e3, 2)
            for cname, ctx in (("serial", d), ("split_default", ds), ("split_gpu_only", gs)):
                ctx.gunzip_buffer(gz)
                t, out = best(lambda: ctx.gunzip_buffer(gz), reps)
                assert out == data
                row[cname + "_ms"] = round(t * 1e3, 2)
            emit(row, fh)
        tmp = tempfile.mkdtemp(prefix="unpack_bench_plain_")
        try:
            build = os.path.join(tmp, "build")
            nfiles = make_package(build, pkg_total, 1)
            arc = os.path.join(tmp, "data.tar.gz")
            with tarfile.open(arc, "w:gz") as t:  # zlib -9, no flush points
                t.add(build, arcname=".")
            # hashes.yaml of what the archive unpacks to (the serial route's tree)
            first = os.path.join(tmp, "first")
            assert d.tar_unpack(arc, first)[0] is None
            from snappy_amd import getHashes
            yaml = getHashes(first, arc, d)
            shutil.rmtree(first)
            row = {"leg": "plain_unpack", "files": nfiles, "bytes": pkg_total, "gz_bytes": os.path.getsize(arc)}
            for cname, ctx in (("serial", d), ("split_default", ds), ("split_gpu_only", gs)):
                times = []
                for r in range(reps):
                    tgt = os.path.join(tmp, "%s%d" % (cname, r))
                    t0 = time.perf_counter()
                    mis, _ = ctx.tar_unpack(arc, tgt, yaml)
                    times.append(time.perf_counter() - t0)
                    assert mis is None
                    shutil.rmtree(tgt)
                st = ctx.unpack_stats()
                row[cname + "_ms"] = round(min(times) * 1e3, 1)
                row[cname + "_segments"] = [st["gpu_segments"], st["segments"]]
                row[cname + "_host_bytes"] = st["host_bytes"]
            raw = open(arc, "rb").read()
            z1, _ = best(lambda: zlib.decompress(raw, 31), reps)
            row["zlib_one_core_inflate_ms"] = round(z1 * 1e3, 1)
            emit(row, fh)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--legs", default="kernel,unpack,plain")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    fh = open(a.out, "w") if a.out else None
    size = (16 << 20) if a.quick else (64 << 20)
    reps = 2 if a.quick else 3
    if "plain" in legs:
        plain(size, reps, 32 << 20 if a.quick else 256 << 20, fh)
    if not legs & {"kernel", "unpack"}:
        return
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
        for name, data in (corpora(size).items() if "kernel" in legs else ()):
            gz = g.gzip_buffer(data)
            g.gunzip_buffer(gz)  # warm: the scratch buffers
            ks = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = g.gunzip_buffer(gz)
                wall = time.perf_counter() - t0
                ks.append((g.unpack_stats()["inflate_ms"], wall))
            assert out == data
            st = g.unpack_stats()
            kms = min(k for k, _ in ks)
            wall = min(w for _, w in ks)
            dw, dout = best(lambda: d.gunzip_buffer(gz), reps)
            assert dout == data
            z1, zout = best(lambda: zlib.decompress(gz, 31), reps)
            assert zout == data
            traffic = len(gz) * 2 + len(data) * 2 * 2 + len(data)  # stream read (scan + decode), slots written + read, bytes out
            emit({"leg": "kernel", "corpus": name, "bytes": len(data), "gz_bytes": len(gz), "segments": st["segments"],
                  "gpu_segments": st["gpu_segments"], "inflate_ms": round(kms, 3), "kernel_gbps": round(len(data) / kms / 1e6, 2),
                  "hbm_fraction": round(traffic / (kms / 1e3) / HBM_PEAK, 4),
                  "gunzip_gpu_only_ms": round(wall * 1e3, 2), "gunzip_default_ms": round(dw * 1e3, 2),
                  "zlib_one_core_ms": round(z1 * 1e3, 2), "default_vs_one_core": round(z1 / dw, 2)}, fh)
        tmp = tempfile.mkdtemp(prefix="unpack_bench_")
        try:
            pkgs = [("config2", 256 << 20 if not a.quick else 32 << 20, "tree")]
            pkgs.append(("text_1GiB", (1 << 30) if not a.quick else (64 << 20), "text"))
            pkgs = pkgs if "unpack" in legs else []
            for label, total, kind in pkgs:
                build = os.path.join(tmp, label, "build")
                if kind == "tree":
                    nfiles = make_package(build, total, 1)
                else:
                    os.makedirs(build)
                    with open(os.path.join(build, "text"), "wb") as f:
                        f.write((corpora(64 << 20)["text"] * (total // (64 << 20)))[:total])
                    nfiles = 1
                arc = os.path.join(tmp, label, "data.tar.gz")
                yaml, _ = d.tar_create(arc, build, build + "/DEBIAN", with_hashes=True)
                gz_bytes = os.path.getsize(arc)
                row = {"leg": "unpack", "package": label, "files": nfiles, "bytes": total, "gz_bytes": gz_bytes}
                for cname, c in (("gpu_only", g), ("default", d)):
                    times = []
                    for r in range(reps):
                        tgt = os.path.join(tmp, label, "%s%d" % (cname, r))
                        t0 = time.perf_counter()
                        mis, _ = c.tar_unpack(arc, tgt, yaml)
                        times.append(time.perf_counter() - t0)
                        assert mis is None
                        shutil.rmtree(tgt)
                    st = c.unpack_stats()
                    row[cname + "_ms"] = round(min(times) * 1e3, 1)
                    row[cname + "_inflate_ms"] = round(st["inflate_ms"], 2)
                    row[cname + "_segments"] = [st["gpu_segments"], st["segments"]]
                # baseline 1: Python zlib + tarfile + snaphash_verify (the archive read twice: unpack, then Verify)
                times = []
                for r in range(reps):
                    tgt = os.path.join(tmp, label, "py%d" % r)
                    t0 = time.perf_counter()
                    with tarfile.open(arc, "r:gz") as t:
                        t.extractall(tgt)
                    assert d.verify(tgt, yaml, arc) is None
                    times.append(time.perf_counter() - t0)
                    shutil.rmtree(tgt)
                row["zlib_tarfile_verify_ms"] = round(min(times) * 1e3, 1)
                # baseline 2: one inflate on one core, nothing else (the reference's gzip.NewReader shape)
                raw = open(arc, "rb").read()
                z1, _ = best(lambda: zlib.decompress(raw, 31), reps)
                row["zlib_one_core_inflate_ms"] = round(z1 * 1e3, 1)
                emit(row, fh)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
