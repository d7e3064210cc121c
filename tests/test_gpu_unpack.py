"""Row f5 on the GPU: snaphash_gunzip_buffer (the GPU inflate: segments decoded side by side, holes filled, the host
decoder for stretches without flush points) and snaphash_tar_unpack (ClickDeb.Unpack with the install-time Verify from
the decoded bytes in HBM), in both configurations (conftest.py snaphash_mode).  The kernels' and the driver's own edges
(far holes, tiny segments, the window in front of a piece, slot capacity, pieces cut inside a segment) are in
tests/test_gpu_inflate_edges.py."""
import gzip
import io
import os
import stat
import tarfile
import zlib

import numpy as np
import pytest

from snappy_amd import Context, _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def corpus(kind, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "zeros":
        return bytes(n)
    if kind == "random":
        return rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
    if kind == "binary":  # the library itself: code and tables
        base = open(os.path.join(ROOT, "snappy_amd", "libsnaphash.so"), "rb").read()
    else:
        words = [bytes(rng.integers(97, 123, size=int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(2000)]
        base = b" ".join(words[int(i)] for i in rng.integers(0, 2000, size=200000))
    reps = n // max(len(base), 1) + 1
    return (base * reps)[:n]


def sync_flush_stream(data, step, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, 31)
    out = [c.compress(data[i:i + step]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(data), step)]
    return b"".join(out) + c.flush()


@pytest.mark.parametrize("kind", ["text", "binary", "random", "zeros"])
def test_gunzip_inverts_gzip_buffer(snaphash_mode, kind):
    with Context(device=0) as c:
        for n in (0, 1, 65535, 65536, 65537, 3 << 20):
            data = corpus(kind, n, seed=n)
            gz = c.gzip_buffer(data)
            assert c.gunzip_buffer(gz) == data, (kind, n)
            st = c.unpack_stats()
            assert st["tar_bytes"] == n and st["gz_bytes"] == len(gz)
            if snaphash_mode == "gpu_only" and kind in ("text", "binary") and n > 65536:
                assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st


@pytest.mark.kernels_only("300 MiB at full size, once")
def test_gunzip_300_mib(snaphash_mode):
    with Context(device=0) as c:
        data = corpus("text", 300 << 20, seed=3)
        gz = c.gzip_buffer(data)
        assert c.gunzip_buffer(gz) == data
        st = c.unpack_stats()
        assert st["gpu_segments"] == st["segments"] >= (300 << 20) // 65536 and st["host_bytes"] == 0, st


def test_python_sync_flush_streams_and_plain_zlib(snaphash_mode):
    data = corpus("text", 5 << 20, seed=5) + corpus("random", 1 << 20, seed=6)
    with Context(device=0) as c:
        gz = sync_flush_stream(data, 32768)
        assert c.gunzip_buffer(gz) == data
        st = c.unpack_stats()
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
        text = data[: 5 << 20]
        plain = gzip.compress(text, 9)  # no flush points: the host's route
        assert c.gunzip_buffer(plain) == text
        st = c.unpack_stats()
        assert st["host_bytes"] == len(text) and st["gpu_segments"] == 0, st
        # zlib -9 stores what does not shrink: its stored blocks end segments too, the text around them is the host's
        assert c.gunzip_buffer(gzip.compress(data, 9)) == data
        two = gzip.compress(data[:100000], 9) + c.gzip_buffer(data)  # concatenated members, one of each kind
        assert c.gunzip_buffer(two) == data[:100000] + data


def test_small_staging_forces_pieces(snaphash_mode):
    data = corpus("text", 6 << 20, seed=8)
    with Context(device=0, staging_bytes=1 << 20) as c:
        gz = c.gzip_buffer(data)
        assert c.gunzip_buffer(gz) == data
        st = c.unpack_stats()
        assert len(gz) > 2 << 20 or st["segments"] >= 96
        assert c.gunzip_buffer(sync_flush_stream(data, 40000, 9)) == data


def test_corrupt_stream_is_eformat_and_ctx_survives(snaphash_mode):
    data = corpus("text", 2 << 20, seed=9)
    with Context(device=0) as c:
        gz = bytearray(c.gzip_buffer(data))
        bad = bytes(gz[:-8]) + bytes([gz[-8] ^ 1]) + bytes(gz[-7:])  # CRC-32
        for b in (bad, bytes(gz[: len(gz) // 2]), b"\x1f\x8b\x08\x00" + bytes(20), b""):
            with pytest.raises(_lib.SnaphashError) as e:
                c.gunzip_buffer(b)
            assert e.value.code == _lib.EFORMAT
        mid = bytearray(gz)
        for k in range(200, len(mid) - 100, len(mid) // 7):
            mid[k] ^= 0x5a
        try:
            out = c.gunzip_buffer(bytes(mid))
            assert out != data
        except _lib.SnaphashError as err:
            assert err.code == _lib.EFORMAT
        assert c.gunzip_buffer(bytes(gz)) == data


def make_tree(root):
    build = os.path.join(root, "build")
    os.makedirs(os.path.join(build, "DEBIAN"))
    os.makedirs(os.path.join(build, "bin"))
    os.makedirs(os.path.join(build, "share", "d" * 120, "e" * 60))
    files = {
        "foo": (b"", 0o644), "bin/run": (b"#!/bin/sh\necho hi\n" * 50, 0o755), "bin/big": (corpus("text", 3 << 20, 1), 0o600),
        "share/blob": (corpus("random", 200000, 2), 0o640), "share/%s/%s/long-name" % ("d" * 120, "e" * 60): (b"deep\n", 0o644),
        "share/zeros": (bytes(150000), 0o640),
    }
    for name, (data, mode) in files.items():
        p = os.path.join(build, name)
        with open(p, "wb") as f:
            f.write(data)
        os.chmod(p, mode)
    os.symlink("/nowhere", os.path.join(build, "broken-link"))
    os.symlink("run", os.path.join(build, "bin", "alias"))
    with open(os.path.join(build, "DEBIAN", "control"), "wb") as f:
        f.write(b"x")
    return build


def tree_view(root):
    out = {}
    for dp, dns, fns in os.walk(root):
        for n in dns + fns:
            p = os.path.join(dp, n)
            st = os.lstat(p)
            rel = os.path.relpath(p, root)
            if stat.S_ISLNK(st.st_mode):
                out[rel] = ("l", os.readlink(p))
            elif stat.S_ISDIR(st.st_mode):
                out[rel] = ("d", stat.S_IMODE(st.st_mode))
            else:
                out[rel] = ("f", stat.S_IMODE(st.st_mode), open(p, "rb").read())
    return out


def test_unpack_reproduces_the_tree_and_matches_tarfile(snaphash_mode, tmp_path):
    build = make_tree(str(tmp_path))
    arc = str(tmp_path / "data.tar.gz")
    with Context(device=0) as c:
        yaml, digest = c.tar_create(arc, build, build + "/DEBIAN", with_hashes=True)
        got = tmp_path / "got"
        mis, dig2 = c.tar_unpack(arc, str(got))
        assert mis is None and dig2 == digest
        st = c.unpack_stats()
        assert st["members"] >= 10
        if snaphash_mode == "gpu_only":
            assert st["gpu_segments"] == st["segments"] and st["host_bytes"] == 0, st
    # tarfile's extraction of the same archive, modes under the same umask
    um = os.umask(0)
    os.umask(um)
    ref = tmp_path / "ref"
    with tarfile.open(arc, "r:gz") as t:
        for m in t.getmembers():
            p = os.path.join(ref, os.path.normpath(m.name))
            os.makedirs(os.path.dirname(p), exist_ok=True)
            if m.isdir():
                os.makedirs(p, exist_ok=True)
                os.chmod(p, m.mode & ~um)
            elif m.issym():
                os.symlink(m.linkname, p)
            else:
                with open(p, "wb") as f:
                    f.write(t.extractfile(m).read())
                os.chmod(p, m.mode & ~um)
    g, r = tree_view(str(got)), tree_view(str(ref))
    assert g == r
    src = tree_view(build)
    src.pop("DEBIAN")
    src.pop("DEBIAN/control")
    assert set(g) == set(src)
    for k, v in src.items():
        assert g[k][0] == v[0] and g[k][-1] == (v[-1] if v[0] != "f" else v[2]) if v[0] != "d" else True
        if v[0] == "f":
            assert g[k][1] == v[1] & ~um


@pytest.fixture
def umask_022():
    old = os.umask(0o022)  # the tree's modes are what a 022 umask leaves alone: the yaml then matches what lands on disk
    yield
    os.umask(old)


def test_unpack_verify_matches_snaphash_verify(snaphash_mode, tmp_path, umask_022):
    build = make_tree(str(tmp_path))
    arc = str(tmp_path / "data.tar.gz")
    with Context(device=0) as c:
        yaml, digest = c.tar_create(arc, build, build + "/DEBIAN", with_hashes=True)
        hbm0 = c.engine_info(0)["hbm_bytes"]
        mis, _ = c.tar_unpack(arc, str(tmp_path / "ok"), yaml)
        assert mis is None
        if snaphash_mode == "gpu_only":  # the decoded tar stays in HBM for Verify: the engine's footprint counts it
            tar_len = len(gzip.decompress(open(arc, "rb").read()))
            assert c.engine_info(0)["hbm_bytes"] - hbm0 >= tar_len, (hbm0, c.engine_info(0), tar_len)
        lines = yaml.split(b"\n")

        def edit(pred, fn):
            out, done = [], False
            for i, ln in enumerate(lines):
                if not done and pred(i, ln):
                    r = fn(ln)
                    done = True
                    if r is None:
                        continue
                    out.extend(r if isinstance(r, list) else [r])
                else:
                    out.append(ln)
            assert done
            return b"\n".join(out)

        def name_at(i):
            return lines[i].startswith(b"- name: ")

        idx_run = lines.index(b"- name: bin/run")
        tampers = {
            "content": edit(lambda i, ln: i > idx_run and ln.startswith(b"  sha512: "), lambda ln: ln[:-1] + (b"0" if ln[-1:] != b"0" else b"1")),
            "size": edit(lambda i, ln: i > idx_run and ln.startswith(b"  size: "), lambda ln: ln + b"1"),
            "mode": edit(lambda i, ln: i > idx_run and ln.startswith(b"  mode: "), lambda ln: ln.replace(b"x", b"-", 1)),
            "archive": edit(lambda i, ln: ln.startswith(b"archive-sha512: "), lambda ln: ln[:-1] + (b"0" if ln[-1:] != b"0" else b"1")),
            "extra record": edit(lambda i, ln: ln == b"- name: foo", lambda ln: [b"- name: bin/zzz", b"  size: 1", b"  sha512: " + b"0" * 128,
                                                                            b"  mode: frw-r--r--", ln]),
        }
        # a record missing from the yaml: drop the record of bin/run (its four lines)
        tampers["missing record"] = b"\n".join(lines[:idx_run] + lines[idx_run + 4:])
        for what, y in tampers.items():
            d = tmp_path / ("t_" + what.replace(" ", "_"))
            mis, _ = c.tar_unpack(arc, str(d), y)
            want = c.verify(str(d), y, arc)
            assert mis is not None and mis == want, (what, mis, want)


def test_dotdot_member_is_econtent_and_stays_inside(snaphash_mode, tmp_path):
    buf = io.BytesIO()
    with tarfile.open(fileobj=buf, mode="w:gz", format=tarfile.GNU_FORMAT) as t:
        for name, data in (("./ok", b"fine"), ("./a/../../escape", b"evil")):
            ti = tarfile.TarInfo(name)
            ti.size = len(data)
            t.addfile(ti, io.BytesIO(data))
    arc = tmp_path / "evil.tar.gz"
    arc.write_bytes(buf.getvalue())
    target = tmp_path / "inside" / "dir"
    with Context(device=0) as c:
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_unpack(str(arc), str(target))
        assert e.value.code == _lib.ECONTENT
        # a name that merely contains ".." is refused as well, as in the reference
        buf = io.BytesIO()
        with tarfile.open(fileobj=buf, mode="w:gz") as t:
            ti = tarfile.TarInfo("./a..b")
            t.addfile(ti, io.BytesIO(b""))
        arc2 = tmp_path / "dots.tar.gz"
        arc2.write_bytes(buf.getvalue())
        with pytest.raises(_lib.SnaphashError) as e:
            c.tar_unpack(str(arc2), str(target))
        assert e.value.code == _lib.ECONTENT
    assert not (tmp_path / "inside" / "escape").exists() and not (tmp_path / "escape").exists()
