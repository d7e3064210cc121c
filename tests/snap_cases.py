"""Builds the .snap packages of the container tests (tests/test_snap_host.py, tests/test_gpu_snap.py) in Python: an ar
writer, tarfile, gzip, bz2, and the oracle's hashes.yaml -- never the code under test, but for the one data.tar form that
is the library's own producer.  A builder, not a test."""
import bz2
import gzip
import hashlib
import io
import os
import tarfile
import zlib

BIG = 70000  # more than one 64 KiB chunk, not a multiple of 512
BIG_NAME = "lib/big.bin"


def ar_pack(members):
    """[(name, bytes)] -> the bytes of an ar archive: global magic, 60-byte headers, data padded to an even offset."""
    out = bytearray(b"!<arch>\n")
    for name, data in members:
        assert len(name) <= 16
        out += b"%-16s%-12d%-6d%-6d%-8s%-10d`\n" % (name.encode(), 0, 0, 0, b"100644", len(data))
        out += data
        if len(data) & 1:
            out += b"\n"
    return bytes(out)


def make_tree(root):
    """The smallest tree that takes every branch: a directory, an empty file, a 1-byte file, a 70 000-byte file, a symlink
    and meta/package.yaml.  -> build_dir"""
    import random
    build = os.path.join(root, "build")
    for d in ("", "bin", "lib", "meta"):
        os.makedirs(os.path.join(build, d), mode=0o755, exist_ok=True)
        os.chmod(os.path.join(build, d), 0o755)
    files = {"bin/empty": b"", "bin/one": b"x", BIG_NAME: random.Random(7).randbytes(BIG),
             "meta/package.yaml": b"name: hello\nversion: 1.0\n"}
    for name, data in files.items():
        p = os.path.join(build, name)
        with open(p, "wb") as f:
            f.write(data)
        os.chmod(p, 0o755 if name == "bin/one" else 0o644)
    os.symlink("one", os.path.join(build, "bin/link"))
    return build


def tar_of(build, extra_first=(), extra_mode=0o644):
    """The tree as tarCreate names it ("./<relative path>", root/root, modes from lstat), in sorted walk order; extra_first:
    (name, bytes) members written in FRONT of the tree's own (an earlier member of a name that comes again), regular
    files of mode extra_mode."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as t:
        for name, data in extra_first:
            ti = tarfile.TarInfo("./" + name)
            ti.size, ti.mode, ti.uname, ti.gname = len(data), extra_mode, "root", "root"
            t.addfile(ti, io.BytesIO(data))
        for dirpath, dirs, files in os.walk(build):
            dirs.sort()
            for nm in sorted(dirs + files):
                p = os.path.join(dirpath, nm)
                ti = t.gettarinfo(p, "./" + os.path.relpath(p, build))
                ti.uid = ti.gid = ti.mtime = 0
                ti.uname = ti.gname = "root"
                if ti.isreg():
                    with open(p, "rb") as f:
                        t.addfile(ti, f)
                else:
                    t.addfile(ti)
    return buf.getvalue()


def tar_files(entries):
    """[(name, bytes)] -> a tar of regular files, names as given."""
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w", format=tarfile.USTAR_FORMAT) as t:
        for name, data in entries:
            ti = tarfile.TarInfo(name)
            ti.size, ti.mode, ti.uname, ti.gname = len(data), 0o644, "root", "root"
            t.addfile(ti, io.BytesIO(data))
    return buf.getvalue()


def gz(data, level=9):
    return gzip.compress(data, level, mtime=0)


def gz_stored(data):
    """One gzip member of stored blocks only: a byte of the payload can be flipped in place."""
    c = zlib.compressobj(0, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def compress(form, tar, ctx=None, build=None, tmp=None):
    """The data.tar member of a form: "pygz" (Python gzip, a plain stream), "bz2" (level 1), "gz2" (two gzip members
    concatenated), "stored", or "libgz" (the library's own producer with its flush points: ctx, build and tmp needed; the
    tar is then the producer's, not `tar`).  -> (member name, bytes)"""
    if form == "pygz":
        return "data.tar.gz", gz(tar)
    if form == "stored":
        return "data.tar.gz", gz_stored(tar)
    if form == "gz2":
        cut = (len(tar) // 2) & ~511
        return "data.tar.gz", gz(tar[:cut]) + gz(tar[cut:], 1)
    if form == "bz2":
        return "data.tar.bz2", bz2.compress(tar, 1)
    assert form == "libgz"
    out = os.path.join(tmp, "libgz-data.tar.gz")
    ctx.tar_create(out, build, build + "/DEBIAN")
    with open(out, "rb") as f:
        return "data.tar.gz", f.read()


def control_tar_gz(yaml, manifest=b"{}\n"):
    ents = [("./manifest", manifest)]
    if yaml is not None:
        ents.insert(0, ("./hashes.yaml", yaml))
    return gz(tar_files(ents))


def hashes_yaml(oracle, build, data_bytes, tmp):
    """The oracle's hashes.yaml over the tree and a data member with these bytes."""
    p = os.path.join(tmp, "oracle-data.bin")
    with open(p, "wb") as f:
        f.write(data_bytes)
    return oracle.hashes_yaml(build, p)


def write_snap(path, data_name, data_bytes, yaml, control_parity=None, lead=()):
    """debian-binary, control.tar.gz (hashes.yaml unless yaml is None, and manifest -- padded until the member's length
    has the parity asked for, so that ar's even-offset padding is taken both ways), then the data member; lead: members
    put in front of all.  -> the length of control.tar.gz"""
    manifest = b"{}\n"
    while True:
        ctl = control_tar_gz(yaml, manifest)
        if control_parity is None or len(ctl) % 2 == control_parity:
            break
        manifest += b"#" + hashlib.sha256(manifest).hexdigest()[:7].encode() + b"\n"  # (filler that does not compress away: the length moves)
    with open(path, "wb") as f:
        f.write(ar_pack(list(lead) + [("debian-binary", b"2.0\n"), ("control.tar.gz", ctl), (data_name, data_bytes)]))
    return len(ctl)


def extract_reference(tar_bytes, target):
    """What tarfile makes of the same tar stream (the tree an unpack must equal)."""
    with tarfile.open(fileobj=io.BytesIO(tar_bytes)) as t:
        try:
            t.extractall(target, filter="fully_trusted")
        except TypeError:  # a tarfile without extraction filters
            t.extractall(target)


def tree_listing(root):
    """{relative name: (type, permission bits, content or link target)} of a tree."""
    import stat
    out = {}
    for dirpath, dirs, files in os.walk(root):
        for nm in dirs + files:
            p = os.path.join(dirpath, nm)
            st = os.lstat(p)
            rel = os.path.relpath(p, root)
            if stat.S_ISLNK(st.st_mode):
                out[rel] = ("l", 0, os.readlink(p))
            elif stat.S_ISDIR(st.st_mode):
                out[rel] = ("d", st.st_mode & 0o777, None)
            else:
                with open(p, "rb") as f:
                    out[rel] = ("f", st.st_mode & 0o777, f.read())
    return out
