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
  --self-check   instead of the legs above: what SNAPHASH_XZ_SELF_CHECK costs.  On each corpus, after one
            warm call, snaphash_xz_buffer and snaphash_xz_buffer_ex with the flag, alternating, five of each: best / median /
            worst of the call, and the check kernel's own time from HIP events (snaphash_get_xz_selfcheck_stats); the bytes
            must be the same.  Then `snaphash -s build-xz` and `snaphash -s build-xz -c` of the 297-file package
            (tools/snap_build_bench.py's), alternating in the same way.
  --no-flag-ab LABEL   instead of the legs above: one run of an A/B of snaphash_xz_buffer WITHOUT the flag between two
            checkouts.  `--tree DIR` names the checkout whose snappy_amd (and libsnaphash.so) is loaded, `--corpora-root DIR`
            the checkout whose files make the corpora: tools/deflate_corpora.py builds "sources" from a tree's own files and
            "binaries" from its own libsnaphash.so, so two checkouts compress different bytes unless both runs name the same
            DIR.  On each corpus (8 MiB) one warm call, then five: best / median / worst, as "build": LABEL.  Alternate the
            two checkouts, three runs each:  xz_bench.py --no-flag-ab parent_run1 --tree P --corpora-root P;
            xz_bench.py --no-flag-ab branch_run1 --corpora-root P; ... (profiles/r16_xz_buffer_parent_ab.jsonl)
  --filter NAME   instead of the legs above: what a BCJ filter (x86, arm, armthumb) in front of LZMA2 buys and costs (DESIGN.md
            sec. 25).  On each corpus (8 MiB): the bytes snaphash_xz_buffer writes without and with the filter, beside
            liblzma's greedy parser (MODE_FAST / MF_HC4 / depth 8) on the same 1 MiB Blocks without and with it -- the gain
            is held against liblzma's, not against ours; the call without and with the filter, alternating, five of each;
            the filter kernels' own time (snaphash_get_xz_filter_stats) beside the chains and chunks kernels of the same
            call (a `snaphash xz -F` child under SNAPHASH_TRACE_XZ=1); and the install side reading the file back.  Then the
            dense launch: snaphash_bcj_device over 1 MiB of E8, one lane's walk, beside sec. 17's one-second bound.
  --level N   instead of the legs above: what level N (1: several candidates a position and a priced parse)
            buys and costs beside level 0.  On each corpus (--quick: 8 MiB) in 1 MiB Blocks: the bytes at both levels beside
            liblzma on the same Blocks -- MODE_FAST / MF_HC4 / depth 8 / nice 273 (the shape of level 0), MODE_NORMAL / MF_HC4 at the
            level's depth / nice 273 (the shape of level 1) and preset 6 (`xz -6 --block-size=1MiB` where the program is installed,
            Python's lzma otherwise): the gain level 0 -> 1 is read against liblzma's own FAST -> NORMAL; the call at both levels,
            alternating, five of each after a warm one; and the chunks kernel's own time and longest launch at both levels
            (a `snaphash xz -L` child under SNAPHASH_TRACE_XZ=1).
  --chain FILTERS instead of the legs above: what a filter chain in front of LZMA2 buys and costs, e.g.
            delta:2 or delta:3,x86,sparc.  On each corpus (8 MiB) and on a generated 16-bit sample ramp: the bytes without and
            with the chain beside liblzma's with the same chain on the same 1 MiB Blocks, the call without and with the
            chain, alternating, five of each, the filter kernels' own time in both directions.  --chain kernels: the filter
            kernels alone, each new filter in both directions, Delta at distances 1, 3 and 256.
usage: tools/xz_bench.py [--quick] [--reps N] [--legs size,time,install,build] [--self-check] [--filter NAME] [--chain FILTERS] [--level N] [--out FILE]
       tools/xz_bench.py --no-flag-ab LABEL [--tree DIR] [--corpora-root DIR] [--out FILE]   (JSON lines on stdout and in FILE; --out appends here)"""
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
# --tree DIR: the checkout whose library is measured (read here, before the library is imported); this one otherwise
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT
sys.path.insert(0, TREE)
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


def three(ms):
    """best / median / worst, in ms"""
    s = sorted(ms)
    return [round(s[0], 2), round(s[len(s) // 2], 2), round(s[-1], 2)]


CHECK_LINE = re.compile(r"self-check: (\d+) chunks, ([\d.]+) ms")


def self_check_legs(g, size, total, fh, tmp, reps=5):
    for name, data in corpora(size).items():
        g.xz_buffer(data)  # one warm call: the scratch
        off, on, kernel, chunks = [], [], [], 0
        for _ in range(reps):
            t0 = time.perf_counter()
            z0 = g.xz_buffer(data)
            off.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            z1 = g.xz_buffer(data, self_check=True)
            on.append((time.perf_counter() - t0) * 1e3)
            st = g.xz_selfcheck_stats()
            assert z0 == z1 and st["chunks"] == g.targz_stats()["chunks"]
            kernel.append(st["ms"])
            chunks = st["chunks"]
        emit({"leg": "self_check", "corpus": name, "bytes": len(data), "chunks": chunks, "reps": reps, "off_ms_best_median_worst": three(off),
              "on_ms_best_median_worst": three(on), "check_kernel_ms_best_median_worst": three(kernel),
              "kernels_ms_on": round(g.targz_stats()["deflate_ms"], 2)}, fh)
    build = package(tmp, total, 297, 5)
    arc = os.path.join(tmp, "data.tar.xz")
    subprocess.run([CLI, "build-xz", build, arc], stdout=subprocess.DEVNULL, check=True)  # one warm call: the page cache
    off, on, kernel, chunks, sizes = [], [], [], 0, set()
    for _ in range(reps):
        for flag, ts in (([], off), (["-c"], on)):
            t0 = time.perf_counter()
            p = subprocess.run([CLI, "-s", "build-xz"] + flag + [build, arc], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, check=True)
            ts.append((time.perf_counter() - t0) * 1e3)
            sizes.add(os.path.getsize(arc))
            if flag:
                m = CHECK_LINE.search(p.stderr)
                chunks = int(m.group(1))
                kernel.append(float(m.group(2)))
    assert len(sizes) == 1
    emit({"leg": "self_check_build", "files": 297, "bytes": total, "chunks": chunks, "reps": reps, "off_ms_best_median_worst": three(off),
          "on_ms_best_median_worst": three(on), "check_kernel_ms_best_median_worst": three(kernel), "xz_bytes": sizes.pop()}, fh)


FILTER_LINE = re.compile(r"filter 0x[0-9A-F]+ ([\d.]+) ms")


def filter_legs(g, d, name_of_filter, fh, tmp, reps=5):
    import numpy as np
    import torch
    fid = _lib.bcj_filter(name_of_filter)
    lz_id = {4: lzma.FILTER_X86, 7: lzma.FILTER_ARM, 8: lzma.FILTER_ARMTHUMB}[fid]
    hc4 = dict(id=lzma.FILTER_LZMA2, dict_size=BLOCK, mode=lzma.MODE_FAST, mf=lzma.MF_HC4, depth=8, nice_len=273, lc=3, lp=0, pb=2)

    def liblzma_blocks(data, chain):
        with ThreadPoolExecutor(16) as ex:
            return sum(ex.map(lambda i: len(lzma.compress(data[i:i + BLOCK], format=lzma.FORMAT_RAW, filters=chain)), range(0, len(data), BLOCK)))

    for name, data in corpora(8 << 20).items():
        g.xz_buffer(data)  # one warm call each: the scratch
        g.xz_buffer(data, filter=fid)
        off, on, kernel = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            z0 = g.xz_buffer(data)
            off.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            z1 = g.xz_buffer(data, filter=fid)
            on.append((time.perf_counter() - t0) * 1e3)
            kernel.append(g.xz_filter_stats()["device_ms"])
        assert lzma.decompress(z0) == data and lzma.decompress(z1) == data
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.xz")
        with open(src, "wb") as f:
            f.write(data)
        p = subprocess.run([CLI, "-g", "xz", src, dst, "-F", name_of_filter], env=dict(os.environ, SNAPHASH_TRACE_XZ="1"), stderr=subprocess.PIPE, text=True, check=True)
        rows = [tuple(float(x) for x in m) for m in TRACE.findall(p.stderr)]
        t_dec, t_dec_max, out = timed(lambda: d.unxz_buffer(z1, bcj=True), 3)
        assert out == data and open(dst, "rb").read() == z1
        fs = d.xz_filter_stats()
        t_gpu, _, out = timed(lambda: g.unxz_buffer(z1, bcj=True), 3)
        assert out == data
        emit({"leg": "filter", "filter": name_of_filter, "corpus": name, "bytes": len(data), "snaphash_xz": len(z0), "snaphash_xz_filter": len(z1),
              "gain_pct": round(100.0 * (len(z1) - len(z0)) / len(z0), 2), "hc4_depth8_1mib_blocks": liblzma_blocks(data, [hc4]),
              "hc4_depth8_1mib_blocks_filter": liblzma_blocks(data, [dict(id=lz_id), hc4]), "reps": reps, "off_ms_best_median_worst": three(off),
              "on_ms_best_median_worst": three(on), "filter_kernels_ms_best_median_worst": three(kernel),
              "chains_ms": round(sum(r[0] for r in rows), 3), "chunks_ms": round(sum(r[1] for r in rows), 3),
              "filter_ms_traced": round(sum(float(x) for x in FILTER_LINE.findall(p.stderr)), 3),
              "unxz_default_ms": round(t_dec * 1e3, 2), "unxz_default_host_blocks": fs["host_blocks"], "unxz_gpu_only_ms": round(t_gpu * 1e3, 2),
              "unxz_gpu_only_filter_kernels_ms": round(g.xz_filter_stats()["device_ms"], 3)}, fh)
    n = 1 << 20  # the dense launch: one lane walks a whole range
    dev = torch.full((n,), 0xE8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = []
    for _ in range(3):
        g.bcj_device(fid, True, dev.data_ptr(), np.array([0], dtype=np.uint64), np.array([n], dtype=np.uint64))
        ms.append(g.stats()["kernel_ms"])
    emit({"leg": "filter_dense_launch", "filter": name_of_filter, "bytes": n, "kernel_ms_best_median_worst": three(ms), "bound_ms": 1000.0}, fh)


def parse_chain(word):
    """"delta:2,x86" -> [("delta", 2), "x86"]"""
    return [("delta", int(w[6:])) if w.startswith("delta:") else w for w in word.split(",")]


def sample_ramp(n):
    """16-bit little-endian samples of a slow sweep with a little noise: what Delta at distance 2 is for"""
    import numpy as np
    t = np.arange(n // 2, dtype=np.float64)
    v = 12000.0 * np.sin(t / 900.0) + 3000.0 * np.sin(t / 37.0) + np.random.default_rng(5).integers(-3, 4, n // 2)
    return v.astype("<i2").tobytes()


def chain_legs(g, d, chain, fh, reps=5):
    """What a filter chain in front of LZMA2 buys and costs, at sec. 25's shape: 8 MiB a corpus in 1 MiB
    Blocks, five alternating calls; the size gain beside liblzma's gain with the same chain on the same Blocks; and on a
    generated 16-bit sample ramp."""
    lz = {"delta": lzma.FILTER_DELTA, "x86": lzma.FILTER_X86, "powerpc": lzma.FILTER_POWERPC, "ia64": lzma.FILTER_IA64, "arm": lzma.FILTER_ARM,
          "armthumb": lzma.FILTER_ARMTHUMB, "sparc": lzma.FILTER_SPARC}
    theirs = [dict(id=lzma.FILTER_DELTA, dist=f[1]) if isinstance(f, tuple) else dict(id=lz[f]) for f in chain]
    hc4 = dict(id=lzma.FILTER_LZMA2, dict_size=BLOCK, mode=lzma.MODE_FAST, mf=lzma.MF_HC4, depth=8, nice_len=273, lc=3, lp=0, pb=2)
    label = ",".join("delta:%d" % f[1] if isinstance(f, tuple) else f for f in chain)

    def liblzma_blocks(data, filters):
        with ThreadPoolExecutor(16) as ex:
            return sum(ex.map(lambda i: len(lzma.compress(data[i:i + BLOCK], format=lzma.FORMAT_RAW, filters=filters)), range(0, len(data), BLOCK)))

    sets = dict(corpora(8 << 20))
    sets["sample_ramp"] = sample_ramp(8 << 20)
    for name, data in sets.items():
        g.xz_buffer(data)  # one warm call each: the scratch
        g.xz_buffer(data, chain=chain)
        off, on, kernel = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            z0 = g.xz_buffer(data)
            off.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            z1 = g.xz_buffer(data, chain=chain)
            on.append((time.perf_counter() - t0) * 1e3)
            kernel.append(g.xz_filter_stats()["device_ms"])
        assert lzma.decompress(z0) == data and lzma.decompress(z1) == data
        t_dec, _, out = timed(lambda: d.unxz_buffer(z1, chains=True), 3)
        assert out == data
        t_gpu, _, out = timed(lambda: g.unxz_buffer(z1, chains=True), 3)
        assert out == data
        undo_ms = g.xz_filter_stats()["device_ms"]
        plain, filt = liblzma_blocks(data, [hc4]), liblzma_blocks(data, theirs + [hc4])
        emit({"leg": "chain", "chain": label, "corpus": name, "bytes": len(data), "snaphash_xz": len(z0), "snaphash_xz_chain": len(z1),
              "gain_pct": round(100.0 * (len(z1) - len(z0)) / len(z0), 2), "hc4_depth8_1mib_blocks": plain, "hc4_depth8_1mib_blocks_chain": filt,
              "liblzma_gain_pct": round(100.0 * (filt - plain) / plain, 2), "reps": reps, "off_ms_best_median_worst": three(off),
              "on_ms_best_median_worst": three(on), "encode_filter_kernels_ms_best_median_worst": three(kernel),
              "unxz_default_ms": round(t_dec * 1e3, 2), "unxz_gpu_only_ms": round(t_gpu * 1e3, 2), "decode_filter_kernels_ms": round(undo_ms, 3)}, fh)


def filter_kernel_legs(g, fh, reps=5):
    """The filter kernels alone (snaphash_xz_filter_device): each new filter in both directions over 8 MiB in 1 MiB ranges."""
    import numpy as np
    import torch
    n = 8 << 20
    data = corpora(n)["binaries"]
    offs, lens = np.arange(0, n, BLOCK, dtype=np.uint64), np.full(n // BLOCK, BLOCK, dtype=np.uint64)
    for filt, param in (("delta", 1), ("delta", 3), ("delta", 256), ("powerpc", 0), ("ia64", 0), ("sparc", 0)):
        for enc in (True, False):
            ms = []
            for _ in range(reps):
                dev = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
                torch.cuda.synchronize()
                g.xz_filter_device(filt, enc, dev.data_ptr(), offs, lens, param=param)
                ms.append(g.stats()["kernel_ms"])
            emit({"leg": "filter_kernels", "filter": filt, "param": param, "direction": "encode" if enc else "decode", "bytes": n, "ranges": len(offs),
                  "launches": g.stats()["launches"], "kernel_ms_best_median_worst": three(ms), "bound_ms": 1000.0}, fh)


LEVEL_DEPTH = {1: 32}  # kXzEncDepthHigh


def level_legs(g, level, size, fh, tmp, reps=5):
    def liblzma_blocks(data, **kw):
        f = dict(id=lzma.FILTER_LZMA2, dict_size=BLOCK, lc=3, lp=0, pb=2, **kw)
        with ThreadPoolExecutor(16) as ex:
            return sum(ex.map(lambda i: len(lzma.compress(data[i:i + BLOCK], format=lzma.FORMAT_RAW, filters=[f])), range(0, len(data), BLOCK)))

    def traced(data, lvl):
        src, dst = os.path.join(tmp, "in"), os.path.join(tmp, "out.xz")
        with open(src, "wb") as f:
            f.write(data)
        p = subprocess.run([CLI, "-g", "xz", src, dst, "-L", str(lvl)], env=dict(os.environ, SNAPHASH_TRACE_XZ="1"), stderr=subprocess.PIPE, text=True, check=True)
        rows = [tuple(float(x) for x in m) for m in TRACE.findall(p.stderr)]
        assert rows
        return open(dst, "rb").read(), round(sum(r[1] for r in rows), 3), round(max(r[3] for r in rows), 3), round(sum(r[0] for r in rows), 3)

    for name, data in corpora(size).items():
        g.xz_buffer(data)  # one warm call each: the scratch
        g.xz_buffer(data, level=level)
        t0s, t1s = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            z0 = g.xz_buffer(data)
            t0s.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            z1 = g.xz_buffer(data, level=level)
            t1s.append((time.perf_counter() - t0) * 1e3)
        assert lzma.decompress(z0) == data and lzma.decompress(z1) == data
        f0, chunks0, longest0, chains0 = traced(data, 0)
        f1, chunks1, longest1, chains1 = traced(data, level)
        assert f0 == z0 and f1 == z1
        fast = liblzma_blocks(data, mode=lzma.MODE_FAST, mf=lzma.MF_HC4, depth=8, nice_len=273)
        normal = liblzma_blocks(data, mode=lzma.MODE_NORMAL, mf=lzma.MF_HC4, depth=LEVEL_DEPTH[level], nice_len=273)
        blk = xz_tool(data, "-6", "--block-size=1MiB")
        six = blk[0] if blk else liblzma_blocks(data, preset=6)
        emit({"leg": "level", "level": level, "corpus": name, "bytes": len(data), "snaphash_xz_level0": len(z0), "snaphash_xz_level": len(z1),
              "gain_pct": round(100.0 * (len(z1) - len(z0)) / len(z0), 2), "liblzma_fast_hc4_8_273": fast,
              "liblzma_normal_hc4_%d_273" % LEVEL_DEPTH[level]: normal, "liblzma_gain_pct": round(100.0 * (normal - fast) / fast, 2),
              "preset6_1mib_blocks": six, "preset6_from": "xz" if blk else "python lzma, raw LZMA2 a Block",
              "over_preset6_pct_level0": round(100.0 * (len(z0) - six) / six, 2), "over_preset6_pct_level": round(100.0 * (len(z1) - six) / six, 2),
              "reps": reps, "level0_ms_best_median_worst": three(t0s), "level_ms_best_median_worst": three(t1s),
              "chains_ms": chains1, "chunks_ms_level0": chunks0, "chunks_ms_level": chunks1, "longest_launch_ms_level0": longest0,
              "longest_launch_ms_level": longest1, "bound_ms": 1000.0}, fh)


def corpora_of(root, size):
    """unpack_bench.corpora with the corpus builders of the checkout at `root`, over that checkout's files."""
    origin = os.path.join(os.path.abspath(root), "tools", "deflate_corpora.py")
    src = open(origin).read().split("depths = ")[0]  # the corpus builders, not the script's own run
    g = {"__name__": "deflate_corpora_src", "__file__": origin}
    exec(compile(src, origin, "exec"), g)
    g["SIZE"] = size
    return {"text": g["text"](), "sources": g["fill"](g["sources"]()), "binaries": g["fill"](g["binaries"]())}


def no_flag_ab(g, label, corpora_root, fh, reps=5):
    for name, data in corpora_of(corpora_root, 8 << 20).items():
        g.xz_buffer(data)  # one warm call: the scratch
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.xz_buffer(data)
            ms.append((time.perf_counter() - t0) * 1e3)
        emit({"leg": "xz_buffer_without_the_flag", "build": label, "corpus": name, "bytes": len(data), "call_ms_best_median_worst": three(ms),
              "kernels_ms": round(g.targz_stats()["deflate_ms"], 2)}, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="size,time,install,build")
    ap.add_argument("--out")
    ap.add_argument("--self-check", action="store_true")
    ap.add_argument("--no-flag-ab", metavar="LABEL")
    ap.add_argument("--filter", metavar="NAME", choices=("x86", "arm", "armthumb"))
    ap.add_argument("--chain", metavar="FILTERS", help="e.g. delta:2 or delta:3,x86,sparc; 'kernels': the filter kernels alone")
    ap.add_argument("--level", type=int, choices=(1,))
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--corpora-root", default=ROOT)
    a = ap.parse_args()
    fh = open(a.out, "a" if a.no_flag_ab else "w") if a.out else None
    legs = a.legs.split(",")
    size = (8 << 20) if a.quick else (64 << 20)
    tmp = tempfile.mkdtemp(prefix="xzenc")
    try:
        if a.no_flag_ab:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
                no_flag_ab(g, a.no_flag_ab, a.corpora_root, fh)
            return
        if a.filter:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
                filter_legs(g, d, a.filter, fh, tmp)
            return
        if a.chain:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
                if a.chain == "kernels":
                    filter_kernel_legs(g, fh)
                else:
                    chain_legs(g, d, parse_chain(a.chain), fh)
            return
        if a.level:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
                level_legs(g, a.level, size, fh, tmp)
            return
        if a.self_check:
            with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
                self_check_legs(g, 8 << 20, (32 << 20) if a.quick else (256 << 20), fh, tmp)
            return
        with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g, Context(device=0, flags=0) as d:
            if set(legs) & {"size", "time", "install"}:
                corpus_legs(g, d, size, a.reps, legs, fh, tmp)
        if "build" in legs:
            build_leg((32 << 20) if a.quick else (256 << 20), a.reps, fh, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
