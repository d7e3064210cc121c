#!/usr/bin/env python3
"""The .snap session and the CRC kernels measured.

  kernel   snaphash_crc32_device on 64 MiB of random bytes in HBM, as one range and as 1 024 ranges, both flavours:
           kernel time (crc_ranges_kernel + crc_fold_kernel, HIP events), GB/s over it, the fraction of the 8 TB/s HBM
           peak (the kernel reads every byte once), and the call's wall time; beside them zlib.crc32 on one core of this
           box over the same bytes (a yardstick for the host, not the library's own crc_parallel, which is not exported)
  snap     a package like config 2 (tools/unpack_bench.py's tree, 256 MiB) as data.tar.gz (the library's producer) and as
           data.tar.bz2 (libbz2 -9) inside a .snap, in both configurations: `audit` and `unpack` (with Verify) through
           the session, beside the route before the session existed -- the data member copied out to a file, then
           snaphash_tar_unpack(_bz2) with the yaml handed in -- five runs each, min and max, so that the spread of the
           old route is there to judge a difference by
  onecore  the .bz2 audit under SNAPHASH_FLAG_GPU_ONLY with the process pinned to one CPU (run this leg under
           `taskset -c 0`): the session's device CRCs against tar_unpack_bz2's host CRCs on the same member
usage: tools/snap_bench.py [--quick] [--legs kernel,snap,onecore] [--out FILE]    (JSON lines on stdout and in FILE)"""
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
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from snappy_amd import Context, _lib  # noqa: E402
from unpack_bench import emit, make_package  # noqa: E402
import snap_cases  # noqa: E402

HBM_PEAK = 8.0e12


def kernel_leg(size, reps, fh):
    import torch
    host = np.random.default_rng(1).integers(0, 256, size, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    raw = host.tobytes()
    t0 = time.perf_counter()
    want = zlib.crc32(raw) & 0xFFFFFFFF
    zlib_ms = (time.perf_counter() - t0) * 1e3
    with Context(device=0, flags=_lib.FLAG_GPU_ONLY) as c:
        for kind, kname in ((_lib.CRC_GZIP, "gzip"), (_lib.CRC_BZIP2, "bzip2")):
            for nr in (1, 1024):
                step = size // nr
                offs = np.arange(nr, dtype=np.uint64) * np.uint64(step)
                lens = np.full(nr, step, dtype=np.uint64)
                c.crc32_device(kind, dev.data_ptr(), offs, lens)  # warm: the scratch
                ks, ws = [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    got = c.crc32_device(kind, dev.data_ptr(), offs, lens)
                    ws.append(time.perf_counter() - t0)
                    ks.append(c.stats()["kernel_ms"])
                if kind == _lib.CRC_GZIP and nr == 1:
                    assert int(got[0]) == want
                k = min(ks)
                emit({"leg": "kernel", "flavour": kname, "ranges": nr, "bytes": size, "kernel_ms": round(k, 4),
                      "kernel_ms_max": round(max(ks), 4), "kernel_gbps": round(size / k / 1e6, 1),
                      "hbm_fraction": round(size / (k / 1e3) / HBM_PEAK, 4), "call_ms": round(min(ws) * 1e3, 3),
                      "zlib_crc32_one_core_ms": round(zlib_ms, 2), "zlib_crc32_one_core_gbps": round(size / zlib_ms / 1e6, 2)}, fh)


def build_snaps(tmp, total, d):
    """-> {form: (snap path, member path, yaml)} for "gz" (the library's producer) and "bz2" (libbz2 -9)."""
    build = os.path.join(tmp, "build")
    nfiles = make_package(build, total, 1)
    out = {}
    arc = os.path.join(tmp, "data.tar.gz")
    yaml, _ = d.tar_create(arc, build, build + "/DEBIAN", with_hashes=True)
    gzb = open(arc, "rb").read()
    tar = d.gunzip_buffer(gzb)
    bzb = bz2.compress(tar, 9)
    arc2 = os.path.join(tmp, "data.tar.bz2")
    with open(arc2, "wb") as f:
        f.write(bzb)
    from snappy_amd import getHashes
    yaml2 = getHashes(build, arc2, d)
    for form, name, data, y, member in (("gz", "data.tar.gz", gzb, yaml, arc), ("bz2", "data.tar.bz2", bzb, yaml2, arc2)):
        path = os.path.join(tmp, form + ".snap")
        snap_cases.write_snap(path, name, data, y)
        out[form] = (path, member, y, len(data))
    return nfiles, out


def runs(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"min_ms": round(min(t), 1), "max_ms": round(max(t), 1), "runs": [round(x, 1) for x in t]}


def snap_leg(total, reps, fh, legs):
    tmp = tempfile.mkdtemp(prefix="snap_bench_")
    try:
        with Context(device=0, flags=0) as d, Context(device=0, flags=_lib.FLAG_GPU_ONLY) as g:
            nfiles, snaps = build_snaps(tmp, total, d)
            k = [0]

            def fresh():
                k[0] += 1
                return os.path.join(tmp, "t%d" % k[0])

            for form, (path, member, yaml, zlen) in snaps.items():
                if "snap" in legs:
                    for cname, c in (("default", d), ("gpu_only", g)):
                        row = {"leg": "snap", "form": form, "config": cname, "files": nfiles, "bytes": total, "member_bytes": zlen}

                        def audit():
                            with c.snap_open(path) as s:
                                assert s.audit()[0] is None
                                row["audit_stats"] = s.stats()

                        def unpack():
                            tgt = fresh()
                            with c.snap_open(path) as s:
                                assert s.unpack(tgt, True)[0] is None
                            shutil.rmtree(tgt)

                        def old_route():  # the member out to a file, then the path-taking entry point with the yaml
                            tgt = fresh()
                            with open(path, "rb") as f:
                                blob = f.read()
                            at = blob.find(b"data.tar")
                            size = int(blob[at + 48:at + 58])
                            out = os.path.join(tmp, "extracted.bin")
                            with open(out, "wb") as f:
                                f.write(blob[at + 60:at + 60 + size])
                            fn = c.tar_unpack if form == "gz" else c.tar_unpack_bz2
                            assert fn(out, tgt, yaml)[0] is None
                            shutil.rmtree(tgt)

                        audit()  # warm: the scratch buffers
                        row["audit"] = runs(audit, reps)
                        row["unpack"] = runs(unpack, reps)
                        row["old_route_unpack"] = runs(old_route, reps)
                        emit(row, fh)
                if "onecore" in legs and form == "bz2":
                    row = {"leg": "onecore", "form": form, "config": "gpu_only", "cpus": len(os.sched_getaffinity(0)), "bytes": total}

                    def audit1():
                        with g.snap_open(path) as s:
                            assert s.audit()[0] is None
                            row["audit_stats"] = s.stats()

                    def host_crc():  # the same decode with the block CRCs on the host thread(s): tar_unpack_bz2 without Verify
                        tgt = fresh()
                        assert g.tar_unpack_bz2(member, tgt)[0] is None
                        shutil.rmtree(tgt)

                    audit1()
                    row["audit_device_crc"] = runs(audit1, reps)
                    row["unpack_bz2_host_crc_no_verify"] = runs(host_crc, reps)
                    emit(row, fh)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--legs", default="kernel,snap")
    a = ap.parse_args()
    legs = set(a.legs.split(","))
    fh = open(a.out, "a") if a.out else None
    if "kernel" in legs:
        kernel_leg((16 << 20) if a.quick else (64 << 20), 5, fh)
    if legs & {"snap", "onecore"}:
        snap_leg((32 << 20) if a.quick else (256 << 20), 3 if a.quick else 5, fh, legs)


if __name__ == "__main__":
    main()
