#!/usr/bin/env python3
"""snaphash_snap_build measured: the 297-file package of tools/bunzip2_bench.py (256 MiB; --quick: 32 MiB) built into a
.snap --reps times without and --reps times with the self-check (SNAPHASH_BUILD_CHECK), alternating, after one warm build
of each.  Per variant: best, median and worst wall time of the call, the spread ((worst - best) / median), the library's
own split (the data pass, the control pass, writing the container), and -- checked builds -- the check kernel's own time
from HIP events and the chunks it walked.  Every build must write the same data member; a `snaphash snap audit` of the
last file closes the run.
--codec xz|bz2 (with --level): the data member in that codec, and beside the two variants a third leg,
"standalone": snaphash_tar_create_xz_ex / _bz2_ex over the same tree with the same options on the same ctx, in turn with
the builds -- what the package costs beyond its data member is the difference.  --corpora: instead of the 297-file
package, one tree per corpus of tools/xz_bench.py (64 MiB; --quick: 8 MiB), the corpus cut into 1 MiB files.
The builds of a tree run in ONE child process under a time limit; the audit in a second.
usage: tools/snap_build_bench.py [--quick] [--reps N] [--codec gz|xz|bz2] [--level N] [--corpora] [--out FILE]
(JSON lines on stdout and in FILE)"""
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
BUILD_LIMIT, AUDIT_LIMIT = 240, 60  # seconds: all builds of a tree; the audit


def step_builds(build, out_dir, reps, codec, level):
    """(child) warm one build of each variant, then reps of each, alternating; with a codec of choice the stand-alone
    producer in turn with them"""
    from snappy_amd import Context
    from snappy_amd.clickdeb import ClickDeb
    rows = {False: [], True: [], "standalone": []}
    digests = set()
    opts = {} if codec == "gz" else dict(codec=codec, **({"level": level} if level is not None else {}))
    with Context(device=0, flags=0) as c:  # the default configuration: what a caller gets
        for k in range(-1, reps):
            for check in (False, True):
                snap = os.path.join(out_dir, "checked.snap" if check else "plain.snap")
                t0 = time.perf_counter()
                w = ClickDeb.create(snap, ctx=c).build(build, check=check, mtime=0, **opts)
                dt = time.perf_counter() - t0
                digests.add(w.archive_digest)
                if k >= 0:
                    rows[check].append(dict(w.build_stats, call_ms=dt * 1e3))
            if codec != "gz":
                create = c.tar_create_xz if codec == "xz" else c.tar_create_bz2
                t0 = time.perf_counter()
                digests.add(create(os.path.join(out_dir, "alone.tar." + codec), build, build + "/DEBIAN", with_hashes=True, level=level or 0)[1])
                dt = time.perf_counter() - t0
                if k >= 0:
                    rows["standalone"].append(dict(c.targz_stats(), call_ms=dt * 1e3))
    # (the .snap files themselves differ from build to build: every build rewrites DEBIAN/hashes.yaml, whose mtime is in control.tar.gz)
    assert len(digests) == 1, "the check changed the data member, or the member is not the stand-alone producer's"
    print(json.dumps({"plain": rows[False], "checked": rows[True], "standalone": rows["standalone"]}))


def summary(name, rows, total, files):
    ms = sorted(r["call_ms"] for r in rows)
    med = statistics.median(ms)
    best = min(rows, key=lambda r: r["call_ms"])
    rec = {"leg": name, "files": files, "bytes": total, "reps": len(rows), "call_ms_best": round(ms[0], 1), "call_ms_median": round(med, 1),
           "call_ms_worst": round(ms[-1], 1), "spread": round((ms[-1] - ms[0]) / med, 3)}
    if name == "standalone":
        rec.update(data_bytes=best["gz_bytes"], tar_bytes=best["tar_bytes"], wall_ms_of_best=round(best["wall_ms"], 1))
        return rec
    rec.update(snap_bytes=best["snap_bytes"], data_bytes=best["data_bytes"], control_bytes=best["control_bytes"], tar_bytes=best["tar_bytes"])
    for k in ("data_ms", "control_ms", "ar_ms"):
        rec[k + "_of_best"] = round(best[k], 1)
    if name == "checked":
        ck = sorted(r["check_ms"] for r in rows)
        rec.update(check_chunks=best["check_chunks"], check_kernel_ms_best=round(ck[0], 2), check_kernel_ms_median=round(statistics.median(ck), 2),
                   check_kernel_ms_worst=round(ck[-1], 2))
    return rec


def corpus_tree(root, data):
    """the corpus as a package: files of 1 MiB under root/build, and DEBIAN/"""
    build = os.path.join(root, "build")
    os.makedirs(os.path.join(build, "DEBIAN"))
    for i in range(0, len(data), 1 << 20):
        d = os.path.join(build, "d%02d" % ((i >> 20) % 8))
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "f%04d" % (i >> 20)), "wb") as f:
            f.write(data[i:i + (1 << 20)])
    return build, (len(data) + (1 << 20) - 1) >> 20


def measure(a, tag, build, tmp, total, files, fh):
    from unpack_bench import emit
    with open(os.path.join(build, "DEBIAN", "control"), "wb") as f:
        f.write(b"Package: bench\nVersion: 1.0\n")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", build, tmp, str(a.reps), a.codec, str(a.level)], stdout=subprocess.PIPE,
                       text=True, check=True, timeout=BUILD_LIMIT)
    rows = json.loads(p.stdout.strip().splitlines()[-1])
    plain, checked = summary("plain", rows["plain"], total, files), summary("checked", rows["checked"], total, files)
    recs = [plain, checked]
    recs.append({"leg": "check_cost", "median_ms": round(checked["call_ms_median"] - plain["call_ms_median"], 1),
                 "of_plain_median": round(checked["call_ms_median"] / plain["call_ms_median"] - 1, 4),
                 "check_kernel_gbps_of_tar": round(checked["tar_bytes"] / (checked["check_kernel_ms_median"] * 1e6), 2)})
    if rows["standalone"]:
        alone = summary("standalone", rows["standalone"], total, files)
        recs.append(alone)
        recs.append({"leg": "package_cost", "median_ms": round(plain["call_ms_median"] - alone["call_ms_median"], 1),
                     "control_plus_container_ms_of_best": round(plain["control_ms_of_best"] + plain["ar_ms_of_best"], 1)})
    for rec in recs:
        emit(dict(rec, **tag), fh)
    r = subprocess.run([CLI, "snap", "-x", "audit", os.path.join(tmp, "checked.snap")] if a.codec == "xz" else
                       [CLI, "snap", "audit", os.path.join(tmp, "checked.snap")], stdout=subprocess.PIPE, text=True, timeout=AUDIT_LIMIT)
    emit(dict({"leg": "audit", "exit": r.returncode, "says": r.stdout.strip()}, **tag), fh)
    return r.returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--codec", choices=("gz", "xz", "bz2"), default="gz")
    ap.add_argument("--level", type=int)
    ap.add_argument("--corpora", action="store_true")
    ap.add_argument("--out")
    ap.add_argument("--step", nargs="+", help=argparse.SUPPRESS)  # the builds, in a process of their own
    a = ap.parse_args()
    if a.step:
        return step_builds(a.step[0], a.step[1], int(a.step[2]), a.step[3], None if a.step[4] == "None" else int(a.step[4]))
    if a.level is not None and a.codec == "gz":
        ap.error("--level is the .xz and the .bz2 producer's (the gzip producer's effort is the ctx's deflate_depth)")
    tag = {} if a.codec == "gz" else {"codec": a.codec, "level": a.level}
    fh = open(a.out, "w") if a.out else None
    tmp = tempfile.mkdtemp(prefix="snapbuild")
    try:
        if a.corpora:
            from xz_bench import corpora_of
            worst = 0
            for name, data in corpora_of(ROOT, (8 << 20) if a.quick else (64 << 20)).items():
                root = os.path.join(tmp, name)
                os.makedirs(root)
                build, files = corpus_tree(root, data)
                worst = max(worst, measure(a, dict(tag, corpus=name), build, root, len(data), files, fh))
                shutil.rmtree(root, ignore_errors=True)
            return 0 if worst == 0 else 1
        from bunzip2_bench import package
        total = (32 << 20) if a.quick else (256 << 20)
        build = package(tmp, total, 297, 5)
        return 0 if measure(a, tag, build, tmp, total, 297, fh) == 0 else 1
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
