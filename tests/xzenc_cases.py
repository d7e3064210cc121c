"""Inputs for the .xz writer's tests (test_xzenc_host.py on the CPU, test_gpu_xzenc.py on the GPU): (name, bytes, block
size) triples, each the smallest at which the thing it is named for can go wrong.  No asserts about the library here.

The Block size is 128 KiB -- the smallest with two LZMA2 chunks of 65 536 bytes -- unless the case is about the Block
size.  No input is larger than three Blocks, but for the one Block of the default size."""
import functools
import random

import xz_cases as X

KiB = 1024
CHUNK = 65536
B = 128 * KiB

DIST_EDGES_SMALL = (1, 2, 3, 4, 5, 127, 128, 129)
DIST_EDGES_FAR = (65535, 65536, 65537, 131000)
PERIODS = (1, 2, 63, 64, 65, 273)
BOUNDARY_PATTERN = 3000


def dist_edges():
    """A 4 KiB random pattern at Block offset 100 and again 65 535, 65 536, 65 537 and 131 000 bytes behind the copy in
    front of it (into an earlier chunk of the same Block: the nearest occurrence is always the previous copy), random
    filler between the copies; then short periods of 1 .. 129 bytes: the distance slots' edges and the reverse trees'
    limit."""
    r = random.Random(77)
    pat = r.randbytes(4096)
    out = bytearray(r.randbytes(100)) + pat
    at = 100
    for d in DIST_EDGES_FAR:
        out += r.randbytes(at + d - len(out))
        at += d
        out += pat
    for d in DIST_EDGES_SMALL:
        out += r.randbytes(9) + X.periodic(d, 300, seed=5)
    return bytes(out)


def boundary(block=B):
    """The same random pattern at the end of Block 0 and at the start of Block 1."""
    pat = X.rnd(BOUNDARY_PATTERN, 91)
    return X.text(block - BOUNDARY_PATTERN, 92) + pat + pat + X.text(5000, 93)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for n in (0, 1, 2, 65535, 65536, 65537, 131071, 131072, 131073, 3 * B + 1):
        out.append(("len_%d" % n, X.text(n, 50 + n % 7), B))
    out.append(("block_64k", X.text(2 * CHUNK + 5, 60), CHUNK))
    out.append(("block_default", X.text((1 << 20) + 100, 61), 0))
    out.append(("block_4m", X.text(70000, 62), 4 << 20))
    out.append(("incompressible", X.rnd(2 * B, 63), B))
    out.append(("mixed_rtrt", X.rnd(CHUNK, 64) + X.text(CHUNK, 65) + X.rnd(CHUNK, 66) + X.text(CHUNK, 67), 256 * KiB))
    out.append(("mixed_tr", X.text(CHUNK, 68) + X.rnd(CHUNK, 69), B))
    for p in PERIODS:
        out.append(("period_%d" % p, X.periodic(p, 70000 - p), B))
    out.append(("all_bytes_twice", bytes(range(256)) * 2, B))
    out.append(("dist_edges", dist_edges(), 512 * KiB))
    out.append(("sprinkled", X.sprinkled(64, 2) + X.sprinkled(1, 2), B))
    out.append(("boundary", boundary(), B))
    return out


def by_name(name):
    return next(c for c in cases() if c[0] == name)
