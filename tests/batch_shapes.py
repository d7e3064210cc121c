"""The calls whose batches tests/golden/batch_traces.json records: stream lengths from a shape's parameters, and the
batches the LIBRARY plans for a shape, read back from its own trace (SNAPHASH_TRACE_BATCHES, a child process on the GPU).
tests/test_batchplan_host.py replays the same shapes through batchplan.cpp on the CPU; tools/record_batch_traces.py
writes the fixture."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_KNOBS = {"new_cap": 1024, "hold_back": 1, "ramp_shift": 3, "ramp_first64": 24, "ramp_growth_pct": 115}
BATCH_RE = re.compile(r"batch (\d+): S (\d+), (\d+) segments, (\d+) bytes, largest share (\d+), (\d+) streams left behind, checksum ([0-9a-f]{16})")
FIELDS = ("S", "segments", "bytes", "largest_share", "left_behind")

# name -> parameters.  source: "files" | "memory"; staging: the Context's staging_bytes; lens: see lengths();
# env: the lab knobs of the call; prior: a call made before it on the same Context (its slots are there already).
SHAPES = {
    "c2_files": {"source": "files", "staging": 256 << 20, "lens": {"kind": "equal", "n": 10001, "size": 1 << 20}},
    "mem_5000x256k": {"source": "memory", "staging": 64 << 20, "lens": {"kind": "equal", "n": 5000, "size": 256 << 10}},
    "files_1250x1m": {"source": "files", "staging": 256 << 20, "lens": {"kind": "equal", "n": 1250, "size": 1 << 20}},
    "zipf_mem": {"source": "memory", "staging": 256 << 20, "lens": {"kind": "zipf", "n": 3000, "top": 64 << 20, "seed": 0xC5}},
    "files_100000x8k": {"source": "files", "staging": 256 << 20, "lens": {"kind": "equal", "n": 100000, "size": 8 << 10}},
    "files_5000x8k": {"source": "files", "staging": 256 << 20, "lens": {"kind": "equal", "n": 5000, "size": 8 << 10}},
    "ragged_files": {"source": "files", "staging": 4 << 20, "lens": {"kind": "ragged", "n": 700, "seed": 31, "top": 1 << 18, "zeros": 5}},
    "ragged_mem": {"source": "memory", "staging": 16 << 20, "lens": {"kind": "ragged", "n": 3000, "seed": 7, "top": 1 << 17, "zeros": 40}},
    "knobs_files": {"source": "files", "staging": 64 << 20, "lens": {"kind": "equal", "n": 6000, "size": 256 << 10},
                    "env": {"SNAPHASH_NEW_PER_BATCH": "0", "SNAPHASH_RAMP_MANY": "8,100", "SNAPHASH_HOLD_BACK": "0"}},
    "slots_there": {"source": "memory", "staging": 256 << 20, "lens": {"kind": "equal", "n": 400, "size": 256 << 10},
                    "prior": {"kind": "equal", "n": 1000, "size": 512 << 10}, "slot_caps": [256 << 20, 256 << 20, 0]},
}
GPU_TEST_SHAPES = ("mem_5000x256k", "files_5000x8k")  # what the -m gpu test runs through the library again


def lengths(p):
    """-> list of stream lengths.  equal: n x size.  zipf: size(r) = clamp(top // r - r % 113, 1 KiB, top), the ranks
    shuffled over the list by PCG64(seed) (a long head: the first is top, the median a few KiB).  ragged: half under
    4 KiB, half up to top, the FIPS 180-4 padding edges and `zeros` empty streams, shuffled by default_rng(seed)."""
    if p["kind"] == "equal":
        return [p["size"]] * p["n"]
    if p["kind"] == "zipf":
        r = np.arange(1, p["n"] + 1, dtype=np.int64)
        size = np.clip(p["top"] // r - (r % 113), 1024, p["top"])
        out = np.empty(p["n"], dtype=np.int64)
        out[np.random.Generator(np.random.PCG64(p["seed"])).permutation(p["n"])] = size
        return [int(x) for x in out]
    if p["kind"] == "ragged":
        rng = np.random.default_rng(p["seed"])
        n, edges = p["n"], [1, 111, 112, 127, 128, 129, 255] + [0] * p["zeros"]
        s = np.concatenate([rng.integers(0, 4096, size=n // 2), rng.integers(4096, p["top"], size=n - n // 2 - len(edges)), edges]).astype(np.int64)
        rng.shuffle(s)
        return [int(x) for x in s]
    raise ValueError(p["kind"])


def knobs_of(env):
    """The lab knobs as batchplan.cpp reads them from these variables (only well-formed values are used here)."""
    k = dict(DEFAULT_KNOBS)
    if "SNAPHASH_NEW_PER_BATCH" in env:
        k["new_cap"] = int(env["SNAPHASH_NEW_PER_BATCH"])
    if "SNAPHASH_HOLD_BACK" in env:
        k["hold_back"] = int(int(env["SNAPHASH_HOLD_BACK"]) != 0)
    if "SNAPHASH_RAMP_SHIFT" in env:
        k["ramp_shift"] = min(max(int(env["SNAPHASH_RAMP_SHIFT"]), 1), 8)
    if "SNAPHASH_RAMP_MANY" in env:
        k["ramp_first64"], k["ramp_growth_pct"] = (int(x) for x in env["SNAPHASH_RAMP_MANY"].split(","))
    return k


def parse_batches(text):
    """The trace lines of one or several calls -> a list of calls, each a list of batches (dicts of FIELDS + checksum)."""
    calls = []
    for m in BATCH_RE.finditer(text):
        if int(m.group(1)) == 0:
            calls.append([])
        assert int(m.group(1)) == len(calls[-1]), "batch numbers out of order"
        calls[-1].append(dict(zip(FIELDS, (int(x) for x in m.groups()[1:6])), checksum=m.group(7)))
    return calls


_CHILD = r"""
import ctypes, json, os, sys, tempfile
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import batch_shapes
from snappy_amd import Context, _lib
shape = batch_shapes.SHAPES[%(name)r]
L = _lib.lib()
with tempfile.TemporaryDirectory() as tmp, Context(staging_bytes=shape["staging"], flags=_lib.FLAG_GPU_ONLY) as c:
    for p in ([shape["prior"]] if "prior" in shape else []) + [shape["lens"]]:
        lens = batch_shapes.lengths(p)
        n = len(lens)
        out = ctypes.create_string_buffer(64 * n)
        if shape["source"] == "memory":  # the plan depends on lengths alone: every stream reads the same buffer
            buf = ctypes.create_string_buffer(max(lens) + 1)
            ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(buf)] * n)
            rc = L.snaphash_sha512_buffers(c._h, ptrs, (ctypes.c_uint64 * n)(*lens), n, out)
        else:  # ... and every stream of a length the same sparse file
            paths = {}
            for ln in set(lens):
                paths[ln] = os.path.join(tmp, "f%%d" %% ln).encode()
                with open(paths[ln], "wb") as f:
                    f.truncate(ln)
            rc = L.snaphash_sha512_files(c._h, (ctypes.c_char_p * n)(*[paths[ln] for ln in lens]), n, out, None)
        assert rc == 0, rc
print("ok")
"""


def library_batches(name):
    """Runs shape `name` through the library on the GPU -> the batches of its last call."""
    shape = SHAPES[name]
    env = dict(os.environ, SNAPHASH_TRACE_BATCHES="1", **shape.get("env", {}))
    r = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT, "name": name}], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=280, env=env)
    err = r.stderr.decode(errors="replace")
    assert r.returncode == 0 and b"ok" in r.stdout, err[-800:]
    calls = parse_batches(err)
    assert len(calls) == (2 if "prior" in shape else 1), err[-800:]
    return calls[-1]
