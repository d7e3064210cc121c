#!/usr/bin/env python3
"""What one DEFLATE block produces: zlib -1 / -6 / -9 on tools/deflate_corpora.py's text, sources and binaries (16 MiB
of each), every block recorded by a serial walk (tests/inflate_blocks_harness.cpp ibh_blocks).  The block mode's slots
(inflate_kernels.h kInflateBlockSlotSyms) and its piece per slot (unpack.inc kBlockPiecePerSlot) are sized from it.
CPU only; needs the built libsnaphash.so (the binaries corpus).
usage: tools/inflate_block_sizes.py [--size MiB] [--out FILE]    (JSON lines on stdout and in FILE)"""
import argparse
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from test_inflate_blocks_host import blocks, load_blocks  # noqa: E402
from unpack_bench import corpora  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16)
    ap.add_argument("--out")
    a = ap.parse_args()
    fh = open(a.out, "w") if a.out else None
    L = load_blocks()
    for name, data in corpora(64 << 20).items():
        data = data[: a.size << 20]
        for level in (1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            raw = c.compress(data) + c.flush()
            bl, end = blocks(L, raw)
            out = np.array([o for _, _, o in bl])
            inb = np.diff(np.array([s for s, _, _ in bl] + [end])) / 8
            types = [t for _, t, _ in bl]
            whole = slice(0, max(1, len(bl) - 1))  # (the last block is cut short by the end of the data)
            rec = {"corpus": name, "level": level, "mib": a.size, "blocks": len(bl), "dynamic": types.count(2), "fixed": types.count(1),
                   "stored": types.count(0), "out_min": int(out[whole].min()), "out_p50": int(np.median(out)),
                   "out_p99": int(np.percentile(out, 99)), "out_max": int(out.max()), "in_min": int(inb[whole].min()),
                   "in_p50": int(np.median(inb))}
            line = json.dumps(rec)
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
