#!/usr/bin/env python3
"""The .xz Check id 10 measured: sha256_ranges_kernel alone and on both sides of the library.

  kernel     snaphash_sha256_device on 64 MiB of random bytes in HBM, cut three ways -- 16 ranges of 4 MiB, 64 of 1 MiB,
             1 024 of 64 KiB: kernel time (HIP events), GB/s over it, MB/s a lane (a range is one chain on one lane: its
             length over the kernel time), the call's wall time; beside it hashlib.sha256 and the library's host SHA-256
             (sha256_core.h through tests/sha256_host_harness.cpp) on the same bytes on one core.  The 4 MiB row is the
             longest launch the library itself issues (a Block of kXzGpuBlockMax): it stands against sec. 17's one second
  unxz       snaphash_unxz_buffer under SNAPHASH_FLAG_GPU_ONLY of the same Blocks (text, liblzma preset 1) with Check 10 and
             with Check 4: the call, the decode and Check kernels together, the Check kernels alone, who took the Checks
  xz         snaphash_xz_buffer_check with Check 10 and with Check 4 on 64 MiB of text, Blocks of 1 MiB, GPU-only
best of --reps with the worst beside it.
usage: tools/sha256_bench.py [--quick] [--reps N] [--legs kernel,unxz,xz] [--out FILE]    (JSON lines on stdout and in FILE)"""
import argparse
import ctypes
import hashlib
import lzma
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from snappy_amd import Context, _lib  # noqa: E402
from unpack_bench import corpora, emit  # noqa: E402
import xz_cases  # noqa: E402
from test_sha256_host import load_sha  # noqa: E402

SHAPES = ((16, 4 << 20), (64, 1 << 20), (1024, 64 << 10))


def best(fn, reps):
    """-> (best seconds, worst seconds, the last result)"""
    t, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return min(t), max(t), out


def kernel_leg(g, size, reps, fh):
    import torch
    host = np.random.default_rng(1).integers(0, 256, size, dtype=np.uint8)
    data = host.tobytes()
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    L = load_sha("-O3")
    out = ctypes.create_string_buffer(32)
    t_py, t_py_max, want = best(lambda: hashlib.sha256(data).digest(), reps)
    t_host, t_host_max, _ = best(lambda: L.sh_sha256(data, len(data), out), reps)
    assert out.raw == want
    emit({"leg": "host", "bytes": size, "hashlib_one_core_ms": round(t_py * 1e3, 2), "hashlib_one_core_ms_max": round(t_py_max * 1e3, 2),
          "hashlib_one_core_mbps": round(size / t_py / 1e6, 1), "library_host_ms": round(t_host * 1e3, 2),
          "library_host_ms_max": round(t_host_max * 1e3, 2), "library_host_mbps": round(size / t_host / 1e6, 1)}, fh)
    for nr, step in SHAPES:
        nr = min(nr, size // step)
        offs = np.arange(nr, dtype=np.uint64) * np.uint64(step)
        lens = np.full(nr, step, dtype=np.uint64)
        got = g.sha256_device(dev.data_ptr(), offs, lens)  # warm: the scratch
        assert got[nr - 1].tobytes() == hashlib.sha256(data[(nr - 1) * step:nr * step]).digest()
        ks, ws = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            g.sha256_device(dev.data_ptr(), offs, lens)
            ws.append(time.perf_counter() - t0)
            ks.append(g.stats()["kernel_ms"])
        k = min(ks)
        emit({"leg": "kernel", "ranges": nr, "range_bytes": step, "bytes": nr * step, "kernel_ms": round(k, 3), "kernel_ms_max": round(max(ks), 3),
              "kernel_gbps": round(nr * step / k / 1e6, 3), "lane_mbps": round(step / k / 1e3, 1), "call_ms": round(min(ws) * 1e3, 3),
              "call_ms_max": round(max(ws) * 1e3, 3)}, fh)


def unxz_leg(g, data, reps, fh):
    for nr, step in SHAPES:
        def one(i):
            return xz_cases.raw_lzma2(data[i:i + step], dict_size=step, preset=1)
        with ThreadPoolExecutor(16) as ex:  # (liblzma drops the GIL)
            blocks = list(ex.map(one, range(0, len(data), step)))
        rec = {"leg": "unxz_gpu_only", "blocks": len(blocks), "block_bytes": step, "bytes": len(data)}
        for label, check in (("sha256", xz_cases.CHECK_SHA256), ("crc64", xz_cases.CHECK_CRC64)):
            z = xz_cases.xz_file(blocks, check, sizes_in_header=True)
            assert g.unxz_buffer(z) == data  # warm: the scratch
            ts, ks, cs = [], [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                g.unxz_buffer(z)
                ts.append(time.perf_counter() - t0)
                ks.append(g.unpack_stats()["inflate_ms"])
                cs.append(g.xz_check_stats()["device_check_ms"])
            st = g.xz_check_stats()
            rec.update({label + "_call_ms": round(min(ts) * 1e3, 2), label + "_call_ms_max": round(max(ts) * 1e3, 2),
                        label + "_kernels_ms": round(min(ks), 2), label + "_check_kernel_ms": round(min(cs), 3),
                        label + "_check_kernel_ms_max": round(max(cs), 3), label + "_device_checks": st["device_" + label],
                        label + "_host_checks": st["host_checks"]})
        emit(rec, fh)


def xz_leg(g, data, reps, fh):
    rec = {"leg": "xz_gpu_only", "bytes": len(data), "block_bytes": 1 << 20}
    g.xz_buffer(data[:1 << 20], check=10)  # warm: the scratch
    for label, check in (("sha256", 10), ("crc64", 4)):
        t, t_max, z = best(lambda: g.xz_buffer(data, check=check), reps)
        assert lzma.decompress(z) == data and z[7] == check
        rec.update({label + "_call_ms": round(t * 1e3, 2), label + "_call_ms_max": round(t_max * 1e3, 2), label + "_xz_bytes": len(z)})
    emit(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--legs", default="kernel,unxz,xz")
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    legs = a.legs.split(",")
    size = (8 << 20) if a.quick else (64 << 20)
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
        if "kernel" in legs:
            kernel_leg(g, size, a.reps, fh)
        if "unxz" in legs or "xz" in legs:
            data = corpora(size)["text"]
            if "unxz" in legs:
                unxz_leg(g, data, a.reps, fh)
            if "xz" in legs:
                xz_leg(g, data, a.reps, fh)


if __name__ == "__main__":
    main()
