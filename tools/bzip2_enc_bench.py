#!/usr/bin/env python3
"""Writing data.tar.bz2 measured: snaphash_bzip2_buffer at level 9 (a block per 719 872 bytes of input, every block coded on
the GPU) on tools/deflate_corpora.py's text, sources and binaries, 64 MiB each (--quick: 8 MiB, one repetition).

  time      the whole call (best of --reps, the worst beside it); the stages' kernels one by one from HIP events (a
            `snaphash bzip2` child under SNAPHASH_TRACE_BZ2=1: CRC, RLE1, BWT, MTF, coding, concatenation, summed over the
            slots, and the longest single launch of each); `bz2.compress(data, 9)` on one core -- what a caller has today
            -- and the same pieces compressed by 16 threads of bz2, the honest parallel baseline
  size      output bytes beside bz2.compress of the whole, bz2 over the same pieces, and zlib -9
  install   snaphash_bunzip2_buffer (default configuration) of this writer's file beside libbz2's file
  build     `snaphash build-bz2` of the 297-file package of tools/bunzip2_bench.py beside `build` and `build-xz`
  --self-check   instead of the legs above: what SNAPHASH_BZ2_SELF_CHECK costs.  On each corpus (8 MiB,
            level 9), after one warm call, snaphash_bzip2_buffer and snaphash_bzip2_buffer_ex with the flag, alternating, five
            of each: best / median / worst of the call, the check's own time from HIP events (snaphash_get_bz2_selfcheck_stats)
            and, from a `snaphash bzip2 -c` child under SNAPHASH_TRACE_BZ2=1, the check's time by stage beside the encoder's;
            the bytes must be the same.  Then `snaphash -s build-bz2` and `snaphash -s build-bz2 -c` of the 297-file package,
            alternating in the same way.
  --no-flag-ab LABEL   instead of the legs above: one run of an A/B of snaphash_bzip2_buffer WITHOUT the flag between two
            checkouts.  `--tree DIR` names the checkout whose snappy_amd (and libsnaphash.so) is loaded, `--corpora-root DIR`
            the checkout whose files make the corpora (tools/xz_bench.py says why).  On each corpus (8 MiB) one warm call, then
            five: best / median / worst, as "build": LABEL.  Alternate the two checkouts, three runs each
            (profiles/r17_bzip2_buffer_parent_ab.jsonl).
Every GPU step -- the timed calls, the traced run, each decode, each build -- is a child process under a time limit sized
to it; host work (bz2, zlib) runs outside them; the first step that fails or runs out ends the run.
usage: tools/bzip2_enc_bench.py [--quick] [--reps N] [--legs time,size,install,build] [--self-check] [--out FILE]
       tools/bzip2_enc_bench.py --no-flag-ab LABEL [--tree DIR] [--corpora-root DIR] [--out FILE]   (JSON lines on stdout and in FILE; --out appends here)"""
import argparse
import bz2
import json
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
# --tree DIR: the checkout whose snappy_amd is loaded (the tools and tests stay this one's)
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[:-1] else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from snappy_amd import Context, _lib  # noqa: E402
from bunzip2_bench import package  # noqa: E402
from unpack_bench import corpora, emit  # noqa: E402
from unxz_bench import timed  # noqa: E402
from xz_bench import corpora_of, three  # noqa: E402

PIECE = (100000 * 9 - 19) * 4 // 5 // 512 * 512
CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
TRACE = re.compile(r"crc ([\d.]+) ms, rle1 ([\d.]+) ms, bwt ([\d.]+) ms, mtf ([\d.]+) ms, code ([\d.]+) ms, concat ([\d.]+) ms")
STAGES = ("crc", "rle1", "bwt", "mtf", "code", "concat")
TRACE_LIMIT, BUILD_LIMIT = 30, 60  # seconds: the traced `snaphash bzip2` child, one `snaphash build*` run


def kernel_trace(data, tmp):
    """The kernels of one `snaphash bzip2` call: summed over its slots, and each stage's longest single launch."""
    src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.bz2")
    with open(src, "wb") as f:
        f.write(data)
    p = subprocess.run([CLI, "-g", "bzip2", src, dst], env=dict(os.environ, SNAPHASH_TRACE_BZ2="1"), stderr=subprocess.PIPE, text=True, check=True,
                       timeout=TRACE_LIMIT)
    rows = [tuple(float(x) for x in m) for m in TRACE.findall(p.stderr)]
    assert rows and bz2.decompress(open(dst, "rb").read()) == data
    rec = {"slots": len(rows)}
    for i, s in enumerate(STAGES):
        rec[s + "_ms"] = round(sum(r[i] for r in rows), 3)
        rec[s + "_longest_launch_ms"] = round(max(r[i] for r in rows), 3)
    return rec


def pieces_16_threads(data):
    """-> (bytes, seconds) of bz2.compress(piece, 9) over the writer's own pieces on 16 threads (libbz2 drops the GIL)."""
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        n = sum(ex.map(lambda o: len(bz2.compress(data[o:o + PIECE], 9)), range(0, len(data), PIECE)))
    return n, time.perf_counter() - t0


def gpu_step(step, limit, *paths):
    """One GPU step in a process of its own, under its own time limit: -> the JSON object it printed last."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step] + list(paths), stdout=subprocess.PIPE, text=True, check=True,
                       timeout=limit)  # (a failure or a step that runs out ends the run)
    return json.loads(p.stdout.strip().splitlines()[-1])


def step_call(src, dst, reps):
    """(child) warm, then `reps` bzip2_buffer calls of the file src; the stream into dst."""
    data = open(src, "rb").read()
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
        g.bzip2_buffer(data[:PIECE])  # warm: the scratch
        t, t_max, z = timed(lambda: g.bzip2_buffer(data), reps)
        st = g.targz_stats()
    open(dst, "wb").write(z)
    print(json.dumps({"s": t, "s_max": t_max, "blocks": st["chunks"], "kernels_ms": st["deflate_ms"]}))


def step_install(path, want, reps):
    """(child) bunzip2_buffer (default configuration) of the file `path`, which decodes to the file `want`."""
    z, data = open(path, "rb").read(), open(want, "rb").read()
    with Context(device=0, flags=0) as d:
        t, t_max, out = timed(lambda: d.bunzip2_buffer(z), reps)
    assert out == data
    print(json.dumps({"s": t, "s_max": t_max}))


def corpus_legs(name, data, reps, legs, fh, tmp):
    """Host work here; every GPU step a child of its own with a limit sized to it: the calls (1 s each at 64 MiB), the traced
    CLI run, each decode."""
    src, ours, libs = os.path.join(tmp, "in"), os.path.join(tmp, "ours.bz2"), os.path.join(tmp, "lib.bz2")
    with open(src, "wb") as f:
        f.write(data)
    call = gpu_step("call", 20 + 10 * reps, src, ours, str(reps))
    z = open(ours, "rb").read()
    assert bz2.decompress(z) == data
    t0 = time.perf_counter()
    whole = bz2.compress(data, 9)
    t_one = time.perf_counter() - t0
    n16, t16 = pieces_16_threads(data)
    t = call["s"]
    if "time" in legs:
        rec = {"leg": "time", "corpus": name, "bytes": len(data), "blocks": call["blocks"], "call_ms": round(t * 1e3, 2),
               "call_ms_max": round(call["s_max"] * 1e3, 2), "call_gbps": round(len(data) / t / 1e9, 3), "kernels_ms": round(call["kernels_ms"], 2),
               "bz2_9_one_core_ms": round(t_one * 1e3, 1), "bz2_9_pieces_16_threads_ms": round(t16 * 1e3, 1),
               "against_one_core": round(t_one / t, 2), "against_16_threads": round(t16 / t, 2)}
        rec.update(kernel_trace(data, tmp))
        emit(rec, fh)
    if "size" in legs:
        emit({"leg": "size", "corpus": name, "bytes": len(data), "snaphash_bzip2": len(z), "bz2_9_whole": len(whole), "bz2_9_pieces": n16,
              "zlib_9": len(zlib.compress(data, 9)), "ratio": round(len(z) / len(data), 4), "against_whole": round(len(z) / len(whole), 4),
              "against_pieces": round(len(z) / n16, 4)}, fh)
    if "install" in legs:
        with open(libs, "wb") as f:
            f.write(whole)
        own = gpu_step("install", 20 + 5 * reps, ours, src, str(reps))
        lib = gpu_step("install", 20 + 5 * reps, libs, src, str(reps))
        emit({"leg": "install", "corpus": name, "bytes": len(data), "bunzip2_own_output_ms": round(own["s"] * 1e3, 2),
              "bunzip2_own_output_ms_max": round(own["s_max"] * 1e3, 2), "bunzip2_libbz2_file_ms": round(lib["s"] * 1e3, 2),
              "bunzip2_libbz2_file_ms_max": round(lib["s_max"] * 1e3, 2)}, fh)


def build_leg(total, reps, fh, tmp):
    build = package(tmp, total, 297, 5)
    rec = {"leg": "build", "files": 297, "bytes": total}
    for verb, arc in (("build", "data.tar.gz"), ("build-xz", "data.tar.xz"), ("build-bz2", "data.tar.bz2")):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            subprocess.run([CLI, verb, build, os.path.join(tmp, arc)], stdout=subprocess.DEVNULL, check=True, timeout=BUILD_LIMIT)
            ts.append(time.perf_counter() - t0)
        key = verb.replace("-", "_")
        rec[key + "_ms"] = round(min(ts) * 1e3, 1)
        rec[key + "_ms_max"] = round(max(ts) * 1e3, 1)
        rec[key + "_bytes"] = os.path.getsize(os.path.join(tmp, arc))
    emit(rec, fh)


CHECK_LINE = re.compile(r"self-check: (\d+) blocks, ([\d.]+) ms")
CHECK_TRACE = re.compile(r"self-check: \d+ blocks: symbols ([\d.]+) ms, link ([\d.]+) ms, ibwt\+rle1 ([\d.]+) ms, compare ([\d.]+) ms")
CHECK_STAGES = ("symbols", "link", "ibwt_rle1", "compare")


def check_trace(data, tmp):
    """The stages of one `snaphash bzip2 -c` call, summed over its slots: the encoder's and the check's."""
    src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.bz2")
    with open(src, "wb") as f:
        f.write(data)
    p = subprocess.run([CLI, "-g", "bzip2", "-c", src, dst], env=dict(os.environ, SNAPHASH_TRACE_BZ2="1"), stderr=subprocess.PIPE, text=True, check=True,
                       timeout=TRACE_LIMIT)
    enc = [tuple(float(x) for x in m) for m in TRACE.findall(p.stderr)]
    chk = [tuple(float(x) for x in m) for m in CHECK_TRACE.findall(p.stderr)]
    assert enc and len(chk) == len(enc)
    rec = {"encoder_" + s + "_ms": round(sum(r[i] for r in enc), 3) for i, s in enumerate(STAGES)}
    rec.update({"check_" + s + "_ms": round(sum(r[i] for r in chk), 3) for i, s in enumerate(CHECK_STAGES)})
    return rec


def self_check_legs(g, size, total, fh, tmp, reps=5):
    for name, data in corpora(size).items():
        g.bzip2_buffer(data)  # one warm call: the scratch
        g.bzip2_buffer(data, self_check=True)  # (and the check's)
        off, on, kernel, blocks = [], [], [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            z0 = g.bzip2_buffer(data)
            off.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            z1 = g.bzip2_buffer(data, self_check=True)
            on.append((time.perf_counter() - t0) * 1e3)
            st = g.bz2_selfcheck_stats()
            assert z0 == z1 and st["blocks"] == g.targz_stats()["chunks"]
            kernel.append(st["ms"])
            blocks = st["blocks"]
        rec = {"leg": "self_check", "corpus": name, "bytes": len(data), "level": 9, "blocks": blocks, "reps": reps, "off_ms_best_median_worst": three(off),
               "on_ms_best_median_worst": three(on), "check_ms_best_median_worst": three(kernel)}
        rec.update(check_trace(data, tmp))
        emit(rec, fh)
    build = package(tmp, total, 297, 5)
    arc = os.path.join(tmp, "data.tar.bz2")
    subprocess.run([CLI, "build-bz2", build, arc], stdout=subprocess.DEVNULL, check=True, timeout=BUILD_LIMIT)  # one warm call: the page cache
    off, on, kernel, blocks, sizes = [], [], [], 0, set()
    for _ in range(reps):
        for flag, ts in (([], off), (["-c"], on)):
            t0 = time.perf_counter()
            p = subprocess.run([CLI, "-s", "build-bz2"] + flag + [build, arc], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, check=True,
                               timeout=BUILD_LIMIT)
            ts.append((time.perf_counter() - t0) * 1e3)
            sizes.add(os.path.getsize(arc))
            if flag:
                m = CHECK_LINE.search(p.stderr)
                blocks = int(m.group(1))
                kernel.append(float(m.group(2)))
    assert len(sizes) == 1
    emit({"leg": "self_check_build", "files": 297, "bytes": total, "blocks": blocks, "reps": reps, "off_ms_best_median_worst": three(off),
          "on_ms_best_median_worst": three(on), "check_ms_best_median_worst": three(kernel), "bz2_bytes": sizes.pop()}, fh)


def no_flag_ab(g, label, corpora_root, fh, reps=5):
    for name, data in corpora_of(corpora_root, 8 << 20).items():
        g.bzip2_buffer(data)  # one warm call: the scratch
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.bzip2_buffer(data)
            ms.append((time.perf_counter() - t0) * 1e3)
        emit({"leg": "bzip2_buffer_without_the_flag", "build": label, "corpus": name, "bytes": len(data), "call_ms_best_median_worst": three(ms),
              "kernels_ms": round(g.targz_stats()["deflate_ms"], 2)}, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="time,size,install,build")
    ap.add_argument("--out")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)  # one GPU step, in a process of its own
    ap.add_argument("--self-check", action="store_true")
    ap.add_argument("--no-flag-ab", metavar="LABEL")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--corpora-root", default=ROOT)
    a = ap.parse_args()
    if a.step:
        return step_call(a.step[1], a.step[2], int(a.step[3])) if a.step[0] == "call" else step_install(a.step[1], a.step[2], int(a.step[3]))
    legs = a.legs.split(",")
    reps = 1 if a.quick else a.reps
    size = (8 << 20) if a.quick else (64 << 20)
    fh = open(a.out, "a" if a.no_flag_ab else "w") if a.out else None
    tmp = tempfile.mkdtemp(prefix="bz2enc")
    try:
        if a.no_flag_ab:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
                no_flag_ab(g, a.no_flag_ab, a.corpora_root, fh)
            return
        if a.self_check:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
                self_check_legs(g, 8 << 20, (32 << 20) if a.quick else (256 << 20), fh, tmp)
            return
        if set(legs) & {"time", "size", "install"}:
            for name, data in corpora(size).items():
                corpus_legs(name, data, reps, legs, fh, tmp)
        if "build" in legs:
            build_leg((32 << 20) if a.quick else (256 << 20), reps, fh, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
