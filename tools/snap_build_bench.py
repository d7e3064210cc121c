#!/usr/bin/env python3
"""snaphash_snap_build measured: the 297-file package of tools/bunzip2_bench.py (256 MiB; --quick: 32 MiB) built into a
.snap --reps times without and --reps times with the self-check (SNAPHASH_BUILD_CHECK), alternating, after one warm build
of each.  Per variant: best, median and worst wall time of the call, the spread ((worst - best) / median), the library's
own split (the data pass, the control pass, writing the container), and -- checked builds -- the check kernel's own time
from HIP events and the chunks it walked.  Every build must write the same data member; a `snaphash snap audit` of the
last file closes the run.
The builds run in ONE child process under a time limit; the audit in a second.
usage: tools/snap_build_bench.py [--quick] [--reps N] [--out FILE]   (JSON lines on stdout and in FILE)"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CLI = os.path.join(ROOT, "snappy_amd", "bin", "snaphash")
BUILD_LIMIT, AUDIT_LIMIT = 240, 60  # seconds: all builds of the run; the audit


def step_builds(build, out_dir, reps):
    """(child) warm one build of each variant, then reps of each, alternating"""
    from snappy_amd import Context
    from snappy_amd.clickdeb import ClickDeb
    rows = {False: [], True: []}
    digests = set()
    with Context(device=0, flags=0) as c:  # the default configuration: what a caller gets
        for k in range(-1, reps):
            for check in (False, True):
                snap = os.path.join(out_dir, "checked.snap" if check else "plain.snap")
                t0 = time.perf_counter()
                w = ClickDeb.create(snap, ctx=c).build(build, check=check, mtime=0)
                dt = time.perf_counter() - t0
                digests.add(w.archive_digest)
                if k >= 0:
                    rows[check].append(dict(w.build_stats, call_ms=dt * 1e3))
    # (the .snap files themselves differ from build to build: every build rewrites DEBIAN/hashes.yaml, whose mtime is in control.tar.gz)
    assert len(digests) == 1, "the check changed the data member"
    print(json.dumps({"plain": rows[False], "checked": rows[True]}))


def summary(name, rows, total):
    ms = sorted(r["call_ms"] for r in rows)
    med = statistics.median(ms)
    best = min(rows, key=lambda r: r["call_ms"])
    rec = {"leg": name, "files": 297, "bytes": total, "reps": len(rows), "call_ms_best": round(ms[0], 1), "call_ms_median": round(med, 1),
           "call_ms_worst": round(ms[-1], 1), "spread": round((ms[-1] - ms[0]) / med, 3), "snap_bytes": best["snap_bytes"],
           "data_bytes": best["data_bytes"], "control_bytes": best["control_bytes"], "tar_bytes": best["tar_bytes"]}
    for k in ("data_ms", "control_ms", "ar_ms"):
        rec[k + "_of_best"] = round(best[k], 1)
    if name == "checked":
        ck = sorted(r["check_ms"] for r in rows)
        rec.update(check_chunks=best["check_chunks"], check_kernel_ms_best=round(ck[0], 2), check_kernel_ms_median=round(statistics.median(ck), 2),
                   check_kernel_ms_worst=round(ck[-1], 2))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)  # the builds, in a process of their own
    a = ap.parse_args()
    if a.step:
        return step_builds(a.step[0], a.step[1], int(a.step[2]))
    from bunzip2_bench import package
    from unpack_bench import emit
    total = (32 << 20) if a.quick else (256 << 20)
    fh = open(a.out, "w") if a.out else None
    tmp = tempfile.mkdtemp(prefix="snapbuild")
    try:
        build = package(tmp, total, 297, 5)
        with open(os.path.join(build, "DEBIAN", "control"), "wb") as f:
            f.write(b"Package: bench\nVersion: 1.0\n")
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", build, tmp, str(a.reps)], stdout=subprocess.PIPE, text=True, check=True,
                           timeout=BUILD_LIMIT)
        rows = json.loads(p.stdout.strip().splitlines()[-1])
        plain, checked = summary("plain", rows["plain"], total), summary("checked", rows["checked"], total)
        emit(plain, fh)
        emit(checked, fh)
        emit({"leg": "check_cost", "median_ms": round(checked["call_ms_median"] - plain["call_ms_median"], 1),
              "of_plain_median": round(checked["call_ms_median"] / plain["call_ms_median"] - 1, 4),
              "check_kernel_gbps_of_tar": round(checked["tar_bytes"] / (checked["check_kernel_ms_median"] * 1e6), 2)}, fh)
        r = subprocess.run([CLI, "snap", "audit", os.path.join(tmp, "checked.snap")], stdout=subprocess.PIPE, text=True, timeout=AUDIT_LIMIT)
        emit({"leg": "audit", "exit": r.returncode, "says": r.stdout.strip()}, fh)
        return 0 if r.returncode == 0 else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
