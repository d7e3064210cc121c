#!/usr/bin/env python3
"""Records the batches the library plans for the shapes of tests/batch_shapes.py (needs the GPU): every shape in a child
process of its own under SNAPHASH_TRACE_BATCHES, a fresh Context each.  With SNAPHASH_LIB pointing at another build of
the same ABI that build is recorded -- tests/golden/batch_traces.json was written this way from the commit before
batchplan.cpp existed, its trace line extended by the checksum for the occasion (tests/golden/README.md says how).

    python tools/record_batch_traces.py OUT.json [shape ...]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_shapes  # noqa: E402


def main():
    out, names = sys.argv[1], sys.argv[2:] or list(batch_shapes.SHAPES)
    doc = {"format": "per batch: " + ", ".join(batch_shapes.FIELDS) + ", checksum", "shapes": {}}
    for name in names:
        batches = batch_shapes.library_batches(name)
        doc["shapes"][name] = dict(batch_shapes.SHAPES[name], batches=[[b[f] for f in batch_shapes.FIELDS] + [b["checksum"]] for b in batches])
        print("%-18s %3d batches, %d segments" % (name, len(batches), sum(b["segments"] for b in batches)), flush=True)
    with open(out, "w") as f:
        f.write("{\n \"format\": %s,\n \"shapes\": {\n" % json.dumps(doc["format"]))
        for i, (name, s) in enumerate(doc["shapes"].items()):
            batches = s.pop("batches")
            f.write("  %s: {\"params\": %s,\n   \"batches\": [\n    %s]}%s\n" % (
                json.dumps(name), json.dumps(s), ",\n    ".join(json.dumps(b) for b in batches), "," if i + 1 < len(doc["shapes"]) else ""))
        f.write(" }\n}\n")


if __name__ == "__main__":
    main()
