"""Trees, victims and mutations for the tests of what a staged pass does when a file changes between the moment its size
is taken and the moment its bytes are read (tests/test_gpu_changed_files.py; DESIGN.md, "What a staged pass does when a
file changes under it").

make_tree(root, seed, shape) builds a tree whose content comes from one numpy generator, and returns a Tree: the
regular files in WALK order (per directory, names in byte order, a directory's content before its next sibling: the
order of filepath.Walk and of the library's walk) with their sizes, and victims by role.  A Mutation changes one file and
knows how to put it back exactly -- bytes, mode, and for the control the new bytes' digest."""
import hashlib
import os
import shutil

import numpy as np

KiB, MiB = 1 << 10, 1 << 20

# the errno a mutation must end the call with (None: the control, no error)
EIO, ENOENT, EISDIR = 5, 2, 21


class Tree:
    def __init__(self, root, files, roles):
        self.root = root
        self.files = files      # [(relative path, size)] in walk order, regular files only, DEBIAN left out
        self.roles = roles      # role -> relative path
        self.index = {rel: i for i, (rel, _) in enumerate(files)}
        self._digests = None

    def path(self, rel):
        return os.path.join(self.root, rel)

    def size(self, rel):
        return self.files[self.index[rel]][1]

    def digests(self):
        """hashlib's SHA-512 of every file, in walk order -- computed once, from the tree as it was built."""
        if self._digests is None:
            self._digests = []
            for rel, _ in self.files:
                with open(self.path(rel), "rb") as f:
                    self._digests.append(hashlib.sha512(f.read()).digest())
        return self._digests


def walk_order(root, skip_top=("DEBIAN",)):
    """Regular files under root in the walk's order, relative paths."""
    out = []

    def visit(d, rel):
        for name in sorted(os.listdir(d), key=os.fsencode):
            if not rel and name in skip_top:
                continue
            p, r = os.path.join(d, name), (rel + "/" + name if rel else name)
            if os.path.isdir(p) and not os.path.islink(p):
                visit(p, r)
            elif os.path.isfile(p) and not os.path.islink(p):
                out.append(r)
    visit(root, "")
    return out


def _write(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(data)
    os.chmod(path, 0o644)


SHAPES = {
    # the tree pass at the smallest staging size (8 MiB): a long file first in walk order that is streamed over every batch;
    # 600 files of 1 to 32 KiB -- the least a file stream is given of a batch (batchplan.h, kMinSegment), so each lies whole
    # in ONE batch, the longer ones in earlier batches; 40 files of 33 to 128 KiB that span batches; a few empty ones; ~33 MiB
    "tree_pass": {"long": 20 * MiB, "dirs": 12, "per_dir": 50, "lo": 1 * KiB, "hi": 32 * KiB, "big": 40, "big_lo": 33 * KiB, "big_hi": 128 * KiB, "empty": 3},
    # the producers at 1 MiB staging: the 40 files of the .gz error test (1 000 .. 200 000 bytes), one long first file of
    # several slots, two empty ones; ~7 MiB
    "producer": {"long": 3 * MiB + 77, "dirs": 4, "per_dir": 10, "lo": 1000, "hi": 200000, "empty": 2},
    # the .xz and .bz2 producers, which write a megabyte in a second or more (the .bz2 producer's slot at 1 MiB of staging is
    # ONE block of 719 872 bytes, a few hundred milliseconds each): the same roles in three slots of 1 MiB, four of
    # 719 872 bytes; ~2.8 MiB
    "producer_small": {"long": 800 * KiB + 77, "dirs": 2, "per_dir": 14, "lo": 1000, "hi": 150000, "empty": 1},
    # the first slot handed over in parts (default staging): 80 MiB, the second part begins inside it
    "in_parts": {"long": 0, "dirs": 4, "per_dir": 5, "lo": 3 * MiB, "hi": 5 * MiB, "empty": 1},
}


def make_tree(root, seed, shape):
    """-> Tree.  Roles: "long" (first in walk order, where the shape has one), "first" (the first regular file behind it --
    the first of the walk where there is no long one), "middle", "last", "empty"."""
    p = SHAPES[shape] if isinstance(shape, str) else shape
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "DEBIAN"))
    _write(os.path.join(root, "DEBIAN", "control"), b"Package: changed-files\n")
    if p["long"]:
        _write(os.path.join(root, "00-long.bin"), rng.bytes(p["long"]))
    n = p["dirs"] * p["per_dir"]
    sizes = rng.integers(p["lo"], p["hi"], size=n)
    for k in range(n):
        # every other file compressible: both block kinds of every encoder occur
        data = rng.bytes(int(sizes[k])) if k % 2 else (b"%06d all work and no play\n" % k) * (int(sizes[k]) // 27 + 1)
        _write(os.path.join(root, "d%02d" % (k // p["per_dir"]), "f%04d.bin" % k), data[:int(sizes[k])])
    for k, size in enumerate(rng.integers(p.get("big_lo", 1), p.get("big_hi", 2), size=p.get("big", 0))):
        _write(os.path.join(root, "d%02d" % (k % p["dirs"]), "b%03d.bin" % k), rng.bytes(int(size)))
    for e in range(p["empty"]):
        _write(os.path.join(root, "d%02d" % ((e * 5 + p["dirs"] // 2) % p["dirs"]), "e%d.empty" % e), b"")
    _write(os.path.join(root, "zz-last.bin"), rng.bytes(int(sizes[0]) | 1))
    rels = walk_order(root)
    files = [(r, os.path.getsize(os.path.join(root, r))) for r in rels]
    regular = [r for r, s in files if s and r != "00-long.bin"]
    roles = {"first": regular[0], "middle": regular[len(regular) // 2], "last": rels[-1],
             "empty": next(r for r, s in files if s == 0)}
    assert roles["last"] == "zz-last.bin" and files[-1][1] > 0
    if p["long"]:
        roles["long"] = "00-long.bin"
        assert rels[0] == "00-long.bin"
    return Tree(root, files, roles)


class Mutation:
    """One change of one file, and its inverse.  errno: what the pass must report (None: no error).  applies(size): a file
    of no bytes cannot shrink, and its rewrite is no change."""
    name = errno = None

    def __init__(self, path):
        self.path = path
        with open(path, "rb") as f:
            self.before = f.read()
        st, up = os.stat(path), os.stat(os.path.dirname(path))
        self.mode = st.st_mode & 0o7777
        self.times = (st.st_atime_ns, st.st_mtime_ns)          # a tar header carries the file's mtime, and its
        self.dir_times = (up.st_atime_ns, up.st_mtime_ns)      # directory's: both are put back with the bytes

    @classmethod
    def applies(cls, size):
        return True

    def restore(self):
        if os.path.isdir(self.path) and not os.path.islink(self.path):
            shutil.rmtree(self.path)
        with open(self.path, "wb") as f:
            f.write(self.before)
        os.chmod(self.path, self.mode)
        os.utime(self.path, ns=self.times)
        os.utime(os.path.dirname(self.path), ns=self.dir_times)
        with open(self.path, "rb") as f:
            assert f.read() == self.before

    def _rewrite(self, data):
        with open(self.path, "wb") as f:
            f.write(data)


class ShrinkByOne(Mutation):
    name, errno = "shrink1", EIO
    applies = classmethod(lambda cls, size: size > 0)

    def apply(self):
        os.truncate(self.path, len(self.before) - 1)


class ShrinkToNothing(Mutation):
    name, errno = "shrink0", EIO
    applies = classmethod(lambda cls, size: size > 0)

    def apply(self):
        os.truncate(self.path, 0)


class GrowByOne(Mutation):
    name, errno = "grow1", EIO

    def apply(self):
        with open(self.path, "ab") as f:
            f.write(b"+")


class Unlink(Mutation):
    name, errno = "unlink", ENOENT

    def apply(self):
        os.unlink(self.path)


class BecomeDirectory(Mutation):
    name, errno = "isdir", EISDIR

    def apply(self):
        os.unlink(self.path)
        os.mkdir(self.path)


class RewriteSameLength(Mutation):
    """The control: other bytes, the same length.  No error; the NEW bytes' digest must come out."""
    name, errno = "rewrite", None
    applies = classmethod(lambda cls, size: size > 0)

    def apply(self):
        self.after = bytes(b ^ 0x5a for b in self.before[:4096]) + self.before[4096:]
        self._rewrite(self.after)


MUTATIONS = {m.name: m for m in (ShrinkByOne, ShrinkToNothing, GrowByOne, Unlink, BecomeDirectory, RewriteSameLength)}
ERRNO_TEXT = {EIO: os.strerror(EIO), ENOENT: os.strerror(ENOENT), EISDIR: os.strerror(EISDIR)}
