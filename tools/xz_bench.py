#!/usr/bin/env python3
"""Writing data.tar.xz measured: snaphash_xz_buffer (Blocks of 1 MiB, LZMA2 chunks of 64 KiB coded side by side on the
GPU) on tools/deflate_corpora.py's text, sources and binaries, 64 MiB each (--quick: 8 MiB).

  size      output bytes beside `xz -6` (the reference's invocation: one Block, 8 MiB dictionary), `xz -6 --block-size=1MiB`,
            liblzma MODE_FAST / MF_HC4 / depth 8 in 1 MiB Blocks (what a greedy parser with the same dictionary reaches:
            the distance to it is the price of resetting the probabilities every 64 KiB plus what the parse loses),
            zlib -9 and this library's own snaphash_gzip_buffer
  time      the whole call (best of --reps, the worst beside it), the kernels one by one from HIP events (a `snaphash xz`
            child under SNAPHASH_TRACE_XZ=1: chains, chunks with its longest single launch, concatenation, CRC-64), beside
            `xz -6` on one core and `xz -6 -T16 --block-size=1MiB` where the xz program is installed (liblzma through
            Python's lzma otherwise, one core)
  install   snaphash_unxz_buffer (default configuration) of our own output against the same bytes as `xz -6`'s one Block
  build     `snaphash build-xz` of the 297-file package of tools/unxz_bench.py beside `snaphash build`
usage: tools/xz_bench.py [--quick] [--reps N] [--legs size,time,install,build] [--out FILE]   (JSON lines on stdout and in FILE)"""
import argparse
import lzma
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from snappy_amd import Context, _lib  # noqa: E402
from bunzip2_bench import package  # noqa: E402
from unpack_bench import corpora, emit  # noqa: E402
from unxz_bench import timed  # noqa: E402

BLOCK = 1 << 20
CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
XZ = shutil.which("xz")
TRACE = re.compile(r"chains ([\d.]+) ms, chunks ([\d.]+) ms in (\d+) launch\(es\) \(longest ([\d.]+)\), concat ([\d.]+) ms, crc64 ([\d.]+) ms")


def xz_tool(data, *args):
    """-> (output bytes, seconds) of the xz program on `data`, or None without it."""
    if not XZ:
        return None
    t0 = time.perf_counter()
    out = subprocess.run([XZ, "--compress", "--stdout"] + list(args), input=data, stdout=subprocess.PIPE, check=True).stdout
    return len(out), time.perf_counter() - t0


def hc4_blocks(data):
    """liblzma MODE_FAST / MF_HC4 / depth 8 over 1 MiB Blocks (raw LZMA2 each): the bytes of the Blocks' data alone."""
    f = dict(id=lzma.FILTER_LZMA2, dict_size=BLOCK, mode=lzma.MODE_FAST, mf=lzma.MF_HC4, depth=8, nice_len=273, lc=3, lp=0, pb=2)
    with ThreadPoolExecutor(16) as ex:
        return sum(ex.map(lambda i: len(lzma.compress(data[i:i + BLOCK], format=lzma.FORMAT_RAW, filters=[f])), range(0, len(data), BLOCK)))


def kernel_trace(data, tmp):
    """The kernels of one `snaphash xz` call, summed over its slots."""
    src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.xz")
    with open(src, "wb") as f:
        f.write(data)
    p = subprocess.run([CLI, "-g", "xz", src, dst], env=dict(os.environ, SNAPHASH_TRACE_XZ="1"), stderr=subprocess.PIPE, text=True, check=True)
    rows = [tuple(float(x) for x in m) for m in TRACE.findall(p.stderr)]
    assert rows and lzma.decompress(open(dst, "rb").read()) == data
    return {"chains_ms": round(sum(r[0] for r in rows), 3), "chunks_ms": round(sum(r[1] for r in rows), 3), "launches": int(sum(r[2] for r in rows)),
            "longest_launch_ms": round(max(r[3] for r in rows), 3), "concat_ms": round(sum(r[4] for r in rows), 3),
            "crc64_ms": round(sum(r[5] for r in rows), 3)}


def corpus_legs(g, d, size, reps, legs, fh, tmp):
    for name, data in corpora(size).items():
        g.xz_buffer(data[:BLOCK])  # warm: the scratch
        t, t_max, z = timed(lambda: g.xz_buffer(data), reps)
        st = g.targz_stats()
        assert lzma.decompress(z) == data
        if "size" in legs:
            rec = {"leg": "size", "corpus": name, "bytes": len(data), "snaphash_xz": len(z), "chunks": st["chunks"], "stored_chunks": st["stored_chunks"],
                   "hc4_depth8_1mib_blocks": hc4_blocks(data), "zlib_9": len(zlib.compress(data, 9)), "snaphash_gzip": len(g.gzip_buffer(data))}
            one, blk = xz_tool(data, "-6"), xz_tool(data, "-6", "--block-size=1MiB")
            rec["xz_6"] = one[0] if one else len(lzma.compress(data, preset=6))
            rec["xz_6_block_1mib"] = blk[0] if blk else None
            rec["below_gzip"] = len(z) < rec["snaphash_gzip"]
            emit(rec, fh)
        if "time" in legs:
            rec = {"leg": "time", "corpus": name, "bytes": len(data), "call_ms": round(t * 1e3, 2), "call_ms_max": round(t_max * 1e3, 2),
                   "call_gbps": round(len(data) / t / 1e9, 3), "kernels_ms": round(st["deflate_ms"], 2)}
            rec.update(kernel_trace(data, tmp))
            one = xz_tool(data, "-6", "-T1")
            if one:
                rec["xz_6_one_core_ms"] = round(one[1] * 1e3, 1)
                rec["xz_6_T16_block_1mib_ms"] = round(xz_tool(data, "-6", "-T16", "--block-size=1MiB")[1] * 1e3, 1)
            else:
                t0 = time.perf_counter()
                lzma.compress(data, preset=6)
                rec["liblzma_6_one_core_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            emit(rec, fh)
        if "install" in legs:
            one = lzma.compress(data, format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64, preset=6)
            t_ours, t_ours_max, out = timed(lambda: d.unxz_buffer(z), reps)
            assert out == data
            t_one, t_one_max, out = timed(lambda: d.unxz_buffer(one), reps)
            assert out == data
            emit({"leg": "install", "corpus": name, "bytes": len(data), "blocks": (len(data) + BLOCK - 1) // BLOCK,
                  "unxz_own_output_ms": round(t_ours * 1e3, 2), "unxz_own_output_ms_max": round(t_ours_max * 1e3, 2),
                  "unxz_xz6_one_block_ms": round(t_one * 1e3, 2), "unxz_xz6_one_block_ms_max": round(t_one_max * 1e3, 2),
                  "gain": round(t_one / t_ours, 2)}, fh)


def build_leg(total, reps, fh, tmp):
    build = package(tmp, total, 297, 5)
    rec = {"leg": "build", "files": 297, "bytes": total}
    for verb, arc in (("build", "data.tar.gz"), ("build-xz", "data.tar.xz")):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            subprocess.run([CLI, verb, build, os.path.join(tmp, arc)], stdout=subprocess.DEVNULL, check=True)
            ts.append(time.perf_counter() - t0)
        key = verb.replace("-", "_")
        rec[key + "_ms"] = round(min(ts) * 1e3, 1)
        rec[key + "_ms_max"] = round(max(ts) * 1e3, 1)
        rec[key + "_bytes"] = os.path.getsize(os.path.join(tmp, arc))
    emit(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="size,time,install,build")
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    legs = a.legs.split(",")
    size = (8 << 20) if a.quick else (64 << 20)
    tmp = tempfile.mkdtemp(prefix="xzenc")
    try:
        with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
            if set(legs) & {"size", "time", "install"}:
                corpus_legs(g, d, size, a.reps, legs, fh, tmp)
        if "build" in legs:
            build_leg((32 << 20) if a.quick else (256 << 20), a.reps, fh, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
