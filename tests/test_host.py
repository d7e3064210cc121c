"""Host-side logic of libsnaphash.so (walk, YAML, modes, LPT) and the C-ABI
surface.  CPU only: nothing here hashes through the library (that needs a GPU);
where a digest is needed to exercise the emitter it is supplied by the oracle,
which is its role as checker."""
import ctypes
import os
import re
import stat

import numpy as np
import pytest

import hostbuild
from conftest import GOLDEN, ROOT
import trees


def test_library_exports_every_declared_symbol(built_lib):
    from snappy_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "snaphash.h")).read()
    declared = set(re.findall(r"\b(snaphash_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS)
    for s in declared:
        assert hasattr(built_lib, s), s
    assert built_lib.snaphash_abi_version() == 5


def test_struct_layouts_match_header(built_lib):
    from snappy_amd import _lib
    assert ctypes.sizeof(_lib.Config) == 56
    assert _lib.Config.devices.offset == 32  # an ABI-1 caller passes struct_size 32: the prefix is unchanged
    assert ctypes.sizeof(_lib.StatsEx) == 112 and _lib.StatsEx.planned_gpu_ms.offset == 64  # ABI 4 callers pass 64
    assert ctypes.sizeof(_lib.Stats) == 56
    assert ctypes.sizeof(_lib.Mismatch) == 8 + 4096
    assert ctypes.sizeof(_lib.Record) == 32
    assert ctypes.sizeof(_lib.EngineInfo) == 72 and _lib.EngineInfo.pinned_bytes.offset == 56  # ABI 3 callers pass 56
    assert ctypes.sizeof(_lib.PlanModel) == 112 and _lib.PlanModel.gpu_seconds.offset == 56  # ABI 4 ...
    assert _lib.PlanModel.fill_rate.offset == 96                                             # ... whose callers pass 96
    assert ctypes.sizeof(_lib.PlanCalib) == 64


def test_no_gpu_means_loud_failure(built_lib):
    """Without a usable gfx950 device the product refuses to start: no CPU fallback."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from snappy_amd import Context, SnaphashError, _lib
    with pytest.raises(SnaphashError) as e:
        Context()
    assert e.value.code == _lib.EDEVICE


def test_product_never_touches_the_oracle():
    """The package must not import, link or shell out to oracle/."""
    pkg = os.path.join(ROOT, "snappy_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="replace").read()
                assert "oracle" not in text.lower() or f == "README.md", os.path.join(dirpath, f)


def test_walk_matches_reference_rules(built_lib, tmp_path):
    from snappy_amd import _lib
    b = tmp_path / "b"
    for d in ("a", "DEBIAN", "DEBIAN-extra", "sub/DEBIAN"):
        (b / d).mkdir(parents=True)
    for f in ("a/x", "a-b", "DEBIANfoo", "DEBIAN/control", "DEBIAN-extra/y", "sub/DEBIAN/kept", "debian"):
        (b / f).write_bytes(f.encode())
    os.symlink("a", str(b / "link-to-dir"))  # dir symlinks are not descended (Lstat)
    recs = _lib.walk(str(b))
    assert [r["name"] for r in recs] == ["a", "a/x", "a-b", "debian", "link-to-dir", "sub", "sub/DEBIAN",
                                         "sub/DEBIAN/kept"]
    by = {r["name"]: r for r in recs}
    assert by["a/x"]["is_regular"] and by["a/x"]["size"] == 3
    assert not by["a"]["is_regular"] and not by["link-to-dir"]["is_regular"]
    assert stat.S_ISLNK(by["link-to-dir"]["st_mode"])
    # trailing slash on the root is tolerated
    assert [r["name"] for r in _lib.walk(str(b) + "/")] == [r["name"] for r in recs]


def test_walk_large_tree_parallel_lstat_keeps_walk_order(built_lib, tmp_path):
    """The walk lists names serially (by directory-entry type) and Lstats in parallel: on a tree big enough for
    several Lstat threads (> 4096 entries) the records must still be filepath.Walk's -- a plain recursive
    sorted-listdir + lstat in Python is the third opinion (names, order, modes, sizes); and a fifo deep inside is
    still the EMODE the serial loop would raise, wherever the threads are."""
    from snappy_amd import _lib, SnaphashError
    rng = np.random.default_rng(4)
    b = tmp_path / "big"
    b.mkdir()
    for d in range(60):
        dn = b / ("d%02d%s" % (d, "-x" if d % 7 == 0 else ""))  # 'd00-x' sorts before 'd00/...' children would: per-directory order
        dn.mkdir()
        for f in range(80):
            (dn / ("f%03d" % f)).write_bytes(b"x" * int(rng.integers(0, 50)))
        if d % 9 == 0:
            (dn / "sub").mkdir()
            (dn / "sub" / "leaf").write_bytes(b"leaf")
            os.symlink("sub", str(dn / "sub-link"))
    (b / "DEBIAN").mkdir()
    (b / "DEBIAN" / "control").write_bytes(b"c")

    def pywalk(path, rel, out):
        st = os.lstat(path)
        if rel and not ("/" + rel).startswith("/DEBIAN"):
            out.append((rel, st.st_mode, st.st_size if stat.S_ISREG(st.st_mode) else 0))
        if stat.S_ISDIR(st.st_mode):
            for name in sorted(os.listdir(path), key=os.fsencode):
                pywalk(os.path.join(path, name), (rel + "/" + name) if rel else name, out)
    want = []
    pywalk(str(b), "", want)
    assert len(want) > 4096
    recs = _lib.walk(str(b))
    assert [(r["name"], r["st_mode"], r["size"]) for r in recs] == want
    os.mkfifo(str(b / "d33" / "f040-pipe"))
    with pytest.raises(SnaphashError) as e:
        _lib.walk(str(b))
    assert e.value.code == _lib.EMODE


def test_walk_fifo_is_unknown_mode(built_lib, tmp_path):
    from snappy_amd import _lib, SnaphashError
    b = tmp_path / "b"
    b.mkdir()
    os.mkfifo(str(b / "pipe"))
    with pytest.raises(SnaphashError) as e:
        _lib.walk(str(b))
    assert e.value.code == _lib.EMODE


def test_emit_golden_yaml_byte_for_byte(built_lib, oracle, tmp_path):
    """snappy/hashes_test.go:89-103 through the product's walk + emitter."""
    from snappy_amd import _lib
    build, tar = trees.make_simple_tree(str(tmp_path))
    recs = _lib.walk(build)
    digs = [oracle.sha512(open(r["path"], "rb").read()) for r in recs if r["is_regular"]]
    y = _lib.emit_yaml(build, oracle.sha512(b""), digs)
    assert y == open(os.path.join(GOLDEN, "hashes_simple.yaml"), "rb").read()


def test_emit_matches_oracle_on_synthetic_tree(built_lib, oracle, tmp_path):
    from snappy_amd import _lib
    build, tar = trees.make_synthetic_tree(str(tmp_path), [0, 1, 127, 128, 129, 4096, 70000, 333, 1000])
    recs = _lib.walk(build)
    digs = [oracle.sha512(open(r["path"], "rb").read()) for r in recs if r["is_regular"]]
    y = _lib.emit_yaml(build, oracle.sha512(open(tar, "rb").read()), digs)
    assert y == oracle.hashes_yaml(build, tar)


def test_emit_empty_and_unsafe(built_lib, oracle, tmp_path):
    from snappy_amd import _lib, SnaphashError
    b = tmp_path / "b"
    b.mkdir()
    assert _lib.emit_yaml(str(b), oracle.sha512(b""), []).endswith(b"files: []\n")
    # what the emitter does not restate is refused, never guessed (tests/test_yaml_names.py has the names it does write)
    for bad in ("0o17", "<<", "0x1p-2", "line\nbreak"):
        (b / bad).write_bytes(b"")
        with pytest.raises(SnaphashError) as e:
            _lib.emit_yaml(str(b), oracle.sha512(b""), [oracle.sha512(b"")])
        assert e.value.code == _lib.ENAME, bad
        os.unlink(str(b / bad))


def test_mode_roundtrip(built_lib):
    from snappy_amd import _lib, SnaphashError, yamlFileMode
    # snappy/hashes_test.go:30-55: fileHash{Mode: 0644|ModeDir} <-> "drw-r--r--"
    assert _lib.mode_string(stat.S_IFDIR | 0o644) == "drw-r--r--"
    assert yamlFileMode.UnmarshalYAML("drw-r--r--") == yamlFileMode(stat.S_IFDIR | 0o644)
    for m in (stat.S_IFREG | 0o644, stat.S_IFREG | 0o755, stat.S_IFDIR | 0o755, stat.S_IFLNK | 0o777,
              stat.S_IFREG | 0o000, stat.S_IFREG | 0o4711):
        s = _lib.mode_string(m)
        assert len(s) == 10
        back = _lib.mode_parse(s)
        assert stat.S_IFMT(back) == stat.S_IFMT(m) and back & 0o777 == m & 0o777
    assert _lib.mode_string(stat.S_IFREG | 0o4755) == "frwxr-xr-x"
    # a perm char counts only if it is the expected letter at that position (hashes.go:81-85)
    assert _lib.mode_parse("fxxxxxxxxx") & 0o777 == 0o111
    for bad in ("", "x---------", "-rw-r--r--"):
        with pytest.raises(SnaphashError):
            _lib.mode_parse(bad)
    for bad in (stat.S_IFIFO, stat.S_IFSOCK, stat.S_IFCHR, stat.S_IFBLK):
        with pytest.raises(SnaphashError):
            _lib.mode_string(bad | 0o600)


def test_lpt_assign(built_lib):
    import numpy as np
    from snappy_amd import _lib, synthetic
    lens = synthetic.zipf_sizes(5000)
    for k in (1, 2, 4, 8):
        s = _lib.lpt_assign(lens, k)
        assert s.min() >= 0 and s.max() < k
        blocks = (lens + np.uint64(17 + 127)) // np.uint64(128)
        loads = np.array([blocks[s == r].sum() for r in range(k)], dtype=np.float64)
        # LPT bound: max load <= mean + largest item
        assert loads.max() <= loads.mean() + blocks.max()
        assert (s == _lib.lpt_assign(lens, k)).all()  # deterministic
    eq = _lib.lpt_assign(np.full(10000, 1 << 20, dtype=np.uint64), 8)
    assert set(np.bincount(eq, minlength=8)) == {1250}


def test_emitted_yaml_is_valid_yaml_for_the_reader_side(built_lib, oracle, tmp_path):
    """Row a8: whatever we emit must unmarshal into hashesYaml{ArchiveSha512, Files[]fileHash}
    (snappy/snapp.go:466-478 reads archive-sha512 back).  PyYAML stands in for yaml.v2's parser."""
    import yaml
    from snappy_amd import _lib
    build, tar = trees.make_synthetic_tree(str(tmp_path), [5, 0, 300, 70000, 12])
    recs = _lib.walk(build)
    digs = [oracle.sha512(open(r["path"], "rb").read()) for r in recs if r["is_regular"]]
    arch = oracle.sha512(open(tar, "rb").read())
    doc = yaml.safe_load(_lib.emit_yaml(build, arch, digs))
    assert set(doc) == {"archive-sha512", "files"} and doc["archive-sha512"] == arch.hex()
    assert [f["name"] for f in doc["files"]] == [r["name"] for r in recs]
    k = 0
    for f, r in zip(doc["files"], recs):
        assert list(f)[0] == "name" and list(f)[-1] == "mode"        # key order name,size,sha512,mode
        assert _lib.mode_parse(f["mode"]) & 0o777 == r["st_mode"] & 0o777
        if r["is_regular"]:
            assert f["size"] == r["size"] and f["sha512"] == digs[k].hex()
            k += 1
        else:
            assert "size" not in f and "sha512" not in f


def test_parse_yaml_reader_side(built_lib):
    """The parser behind snaphash_verify: yaml.v2's renderings of hashesYaml, CPU only."""
    from snappy_amd import _lib, SnaphashError
    golden = open(os.path.join(GOLDEN, "hashes_simple.yaml"), "rb").read()
    arch, recs = _lib.parse_yaml(golden)
    assert arch.startswith("cf83e135") and len(arch) == 128
    assert [r["name"] for r in recs] == ["bin", "bin/bar", "broken-link", "foo"]
    assert [r["is_regular"] for r in recs] == [False, True, False, True]
    assert recs[1]["size"] == 4 and recs[1]["sha512"].startswith("cc06808c") and recs[3]["size"] == 0
    assert stat.S_ISDIR(recs[0]["st_mode"]) and stat.S_ISLNK(recs[2]["st_mode"]) and recs[2]["st_mode"] & 0o777 == 0o777
    # snappy/hashes_test.go:30-33 as a one-record list; quoted scalars as yaml.v2 writes odd names; xattr ignored
    text = (b"archive-sha512: F00F00\nfiles:\n- name: \"123\"\n  size: 10\n  mode: drw-r--r--\n"
            b"- name: 'it''s'\n  mode: frw-r--r--\n  size: 0\n  sha512: abc\n  xattr:\n    user.k: v\n"
            b"- name: \"tab\\there \\u00e9\"\n  mode: lrwxrwxrwx\n")
    arch, recs = _lib.parse_yaml(text)
    assert arch == "F00F00"  # snappy/snapp_test.go:159-170 TestLocalSnapHash: carried as a string
    assert [r["name"] for r in recs] == ["123", "it's", "tab\there \u00e9"]
    assert recs[0]["size"] == 10 and stat.S_ISDIR(recs[0]["st_mode"]) and recs[0]["st_mode"] & 0o777 == 0o644
    assert recs[1]["sha512"] == "abc" and recs[1]["is_regular"]
    assert _lib.parse_yaml(b"{}\n") == ("", [])                       # snappy/common_test.go:77-80
    assert _lib.parse_yaml(b"archive-sha512: ab\nfiles: []\n") == ("ab", [])
    for bad in (b"files:\n- name: x\n", b"files:\n- mode: frw-r--r--\n", b"files:\n- name: x\n  mode: ''\n",
                b"files:\n- name: x\n  mode: qrw-r--r--\n", b"files:\n- name: x\n  size: ten\n  mode: frw-r--r--\n",
                b"- name: x\n", b"files: 3\n"):
        with pytest.raises(SnaphashError) as e:
            _lib.parse_yaml(bad)
        assert e.value.code == _lib.EPARSE, bad


def test_a_big_hashes_yaml_is_parsed_in_ranges_and_comes_out_the_same(built_lib):
    """hostpass.cpp parse_yaml: a document of 20 000 lines and more is parsed in ranges that begin at a list item, a thread
    each.  Names that are quoted, folded over several lines, or look like list items inside their continuation lines sit
    where the cuts fall; a further top-level key after the list, or a broken line, sends the text down the serial way."""
    import random
    from snappy_amd import _lib, SnaphashError
    rng = random.Random(12)
    want, lines = [], ["archive-sha512: " + "ab" * 64, "files:"]
    for i in range(15000):
        kind = rng.randrange(12)
        if kind == 0:
            name = "d%05d/" % i + " ".join("word%d" % rng.randrange(1000) for _ in range(30))  # folded by the emitter past column 80
            folded = ["- name: " + name[:60].rsplit(" ", 1)[0]]
            rest = name[len(folded[0]) - 8 + 1:]
            while rest:
                cut = rest[:70].rsplit(" ", 1)[0] if len(rest) > 70 and " " in rest[:70] else rest
                folded.append("    " + cut)
                rest = rest[len(cut) + 1:]
            lines += folded
        elif kind == 1:
            name = "d%05d/it's - name: not an item" % i
            lines.append("- name: '" + name.replace("'", "''") + "'")
        elif kind == 2:
            name = "d%05d/tab\there" % i
            lines.append('- name: "d%05d/tab\\there"' % i)
        else:
            name = "d%05d/f%07d.bin" % (i // 100, i)
            lines.append("- name: " + name)
        if kind == 3:
            want.append((name, None, "drwxr-xr-x"))
            lines.append("  mode: drwxr-xr-x")
        else:
            size = rng.randrange(1 << 40)
            hexd = "%0128x" % rng.getrandbits(512)
            want.append((name, (size, hexd), "frw-r--r--"))
            lines += ["  size: %d" % size, "  sha512: " + hexd, "  mode: frw-r--r--"]
            if kind == 4:
                lines += ["  xattr:", "    user.k: v", "    - name: inside a nested block"]
    text = ("\n".join(lines) + "\n").encode()
    assert len(lines) > 40000

    def check(t):
        arch, recs = _lib.parse_yaml(t)
        assert arch == "ab" * 64 and len(recs) == len(want)
        for r, (name, fs, mode) in zip(recs, want):
            assert r["name"] == name, (r["name"], name)
            assert _lib.mode_string(r["st_mode"]) == mode
            if fs:
                assert (r["size"], r["sha512"]) == fs
    check(text)
    check(text.replace(b"\n", b"\r\n"))
    check(text + b"later-key: 1\n")                          # not only list items after `files:`: the serial way, same records
    check(b"# a comment\n---\n" + text)
    broken = text.replace(b"  mode: frw-r--r--\n- name: d00120", b"  mode: ?rw-r--r--\n- name: d00120", 1)
    assert broken != text
    with pytest.raises(SnaphashError) as e:
        _lib.parse_yaml(broken)
    assert e.value.code == _lib.EPARSE


def test_hostpass_under_asan_and_ubsan(tmp_path):
    """hostpass.cpp (walk, emitter, parser of untrusted hashes.yaml, LPT) built with
    AddressSanitizer + UBSan and driven with 20 000 mutated documents."""
    exe = hostbuild.sanitized(["tests/asan_hostpass.cpp"] + ["snappy_amd/csrc/" + f for f in
                              ("hostpass.cpp", "yamlscalar.cpp", "walk.cpp", "hostfill.cpp", "planner.cpp")])
    build, tar = trees.make_synthetic_tree(str(tmp_path / "t"), [5, 0, 300, 70000, 12, 1, 2, 3])
    assert "asan driver ok" in hostbuild.run_sanitized(exe, [build, os.path.join(GOLDEN, "hashes_simple.yaml")]).stdout



def test_threaded_host_code_under_tsan(tmp_path):
    """What the library runs on more than one host thread -- the level-wise walk, the ranged YAML emitter, the pool of
    staging-fill threads, the read-ahead reader of a long host-hashed file -- built with ThreadSanitizer
    (tests/tsan_host.cpp): no report, every result equal to the single-threaded one."""
    exe = hostbuild.sanitized(["tests/tsan_host.cpp"] + ["snappy_amd/csrc/" + f for f in
                              ("hostpass.cpp", "yamlscalar.cpp", "walk.cpp", "hostfill.cpp", "hostsha.cpp", "planner.cpp")], sanitize="thread")
    build = tmp_path / "build"
    for d in range(40):
        for e in range(3):
            p = build / ("d%02d" % d) / ("e%d" % e)
            p.mkdir(parents=True)
            for f in range(90):  # 10 800 files: their hashes.yaml is long enough for the parser's ranges too
                (p / ("f%03d" % f)).write_bytes(b"x" * (f * 13))
    big = tmp_path / "big.bin"
    big.write_bytes(os.urandom(1 << 20) * 40)
    assert "tsan driver ok" in hostbuild.run_sanitized(exe, [build, big], sanitize="thread").stdout


_UNLISTABLE_CHILD = r'''
import ctypes, sys
d, build, tar = sys.argv[1], sys.argv[2].encode(), sys.argv[3].encode()
L = ctypes.CDLL(d + "/libsnaphash.so")
O = ctypes.CDLL(d + "/liboracle.so")
class Record(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("st_mode", ctypes.c_uint32), ("is_regular", ctypes.c_int32),
                ("size", ctypes.c_int64), ("path", ctypes.c_char_p)]
L.snaphash_walk.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p)]
L.snaphash_records_count.argtypes = [ctypes.c_void_p]; L.snaphash_records_count.restype = ctypes.c_size_t
L.snaphash_records_get.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Record)]
h = ctypes.c_void_p()
rc = L.snaphash_walk(build, ctypes.byref(h))
print("walk rc", rc)
r = Record()
for i in range(L.snaphash_records_count(h)):
    L.snaphash_records_get(h, i, ctypes.byref(r))
    print("rec", r.name.decode())
O.oracle_hashes_yaml.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_int)]
p, n, en = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
rc = O.oracle_hashes_yaml(build, tar, ctypes.byref(p), ctypes.byref(n), ctypes.byref(en))
print("oracle rc", rc)
for line in ctypes.string_at(p.value, n.value).decode().splitlines():
    if line.startswith("- name:"):
        print("orc", line[len("- name: "):])
'''


def test_unlistable_directory_is_emitted_twice_and_the_walk_goes_on(built_lib, oracle, tmp_path):
    """filepath.Walk hands a ReadDir error to the callback in a SECOND call for the directory; writeHashes' callback
    ignores its err argument (snappy/build.go:228) and tarCreate's shadows it (clickdeb/deb.go:285-286): the entry
    is emitted again and the walk continues.  No reference test covers it (restated from path/filepath's walk()).
    Run as an unprivileged child when the suite runs as root (root lists a mode-000 directory)."""
    import shutil
    import subprocess
    import sys
    import tempfile
    from snappy_amd import _lib
    work = tempfile.mkdtemp(prefix="snaphash_unlistable_", dir="/tmp")
    try:
        os.chmod(work, 0o755)
        shutil.copy(_lib.LIB_PATH, work)
        shutil.copy(os.path.join(ROOT, "oracle", "liboracle.so"), work)
        b = os.path.join(work, "build")
        os.makedirs(os.path.join(b, "a"))
        os.makedirs(os.path.join(b, "locked", "inner"))
        os.makedirs(os.path.join(b, "z"))
        for rel in ("a/f", "locked/inner/g", "z/h"):
            with open(os.path.join(b, rel), "w") as f:
                f.write(rel)
        tar = os.path.join(work, "data.tar.gz")
        open(tar, "w").close()
        os.chmod(os.path.join(b, "locked"), 0o000)
        for dp, dn, fn in os.walk(work):
            for x in dn + fn:
                if x != "locked":
                    os.chmod(os.path.join(dp, x), 0o755)

        def drop():
            if os.geteuid() == 0:
                os.setgid(65534)
                os.setuid(65534)
        r = subprocess.run([sys.executable, "-c", _UNLISTABLE_CHILD, work, b, tar], preexec_fn=drop, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert "walk rc 0" in out and "oracle rc 0" in out
        want = ["a", "a/f", "locked", "locked", "z", "z/h"]
        assert [l[4:] for l in out if l.startswith("rec ")] == want
        assert [l[4:] for l in out if l.startswith("orc ")] == want
    finally:
        os.chmod(os.path.join(work, "build", "locked"), 0o755)
        shutil.rmtree(work, ignore_errors=True)


def test_numa_probe_on_a_fake_sysfs(built_lib, tmp_path):
    """Engine -> NUMA node -> CPU set, as snaphash_init derives it (hostfill.cpp), on a two-socket sysfs tree built
    here: GPUs 0-3 hang off node 0, GPUs 4-7 off node 1."""
    from snappy_amd import _lib
    sysfs = tmp_path / "sys"
    gpus = ["0000:05:00.0", "0000:15:00.0", "0000:65:00.0", "0000:75:00.0", "0000:85:00.0", "0000:95:00.0", "0000:e5:00.0", "0000:f5:00.0"]
    for k, bdf in enumerate(gpus):
        d = sysfs / "bus" / "pci" / "devices" / bdf
        d.mkdir(parents=True)
        (d / "numa_node").write_text("%d\n" % (k // 4))
    (sysfs / "bus" / "pci" / "devices" / "0000:aa:00.0").mkdir()
    (sysfs / "bus" / "pci" / "devices" / "0000:aa:00.0" / "numa_node").write_text("-1\n")
    for node, cl in ((0, "0-63,128-191\n"), (1, "64-127,192-255\n")):
        d = sysfs / "devices" / "system" / "node" / ("node%d" % node)
        d.mkdir(parents=True)
        (d / "cpulist").write_text(cl)
    for k, bdf in enumerate(gpus):
        node, cpus = _lib.numa_probe(str(sysfs), bdf.upper() if k % 2 else bdf)  # HIP may spell the id in upper case
        assert node == k // 4
        lo = 64 * node
        assert cpus == list(range(lo, lo + 64)) + list(range(128 + lo, 128 + lo + 64))
    # four engines on a node: disjoint slices, whole cores (a CPU and its SMT sibling, 128 apart here, stay together)
    L = _lib.lib()
    seen = set()
    for node in (0, 1):
        for pos in range(4):
            n = ctypes.c_size_t()
            buf = (ctypes.c_int32 * 256)()
            assert L.snaphash_numa_slice(str(sysfs).encode(), node, pos, 4, buf, 256, ctypes.byref(n)) == 0
            mine = list(buf[:n.value])
            lo = 64 * node + 16 * pos
            assert mine == list(range(lo, lo + 16)) + list(range(128 + lo, 128 + lo + 16))
            assert not (seen & set(mine))
            seen |= set(mine)
    assert seen == set(range(256))
    assert _lib.numa_probe(str(sysfs), "0000:aa:00.0") == (-1, [])   # sysfs says "no node"
    assert _lib.numa_probe(str(sysfs), "0000:bb:00.0") == (-1, [])   # unknown function
    assert _lib.numa_probe("/nonexistent", gpus[0]) == (-1, [])


def test_large_tree_is_walked_and_written_in_parallel_like_the_serial_loop(built_lib, oracle, tmp_path):
    """9 000 records: the walk lists the directories of a level on several threads and Lstats in ranges, the emitter
    writes ranges of records on several threads and joins them in order -- the bytes must be what the oracle's serial
    loop writes (walk order, digests attached to the right records across the range boundaries, odd names included)."""
    import hashlib
    from snappy_amd import _lib
    b = tmp_path / "build"
    (b / "DEBIAN").mkdir(parents=True)
    (b / "DEBIAN" / "control").write_text("x")
    n = 0
    for d in range(60):
        sub = b / ("dir%03d" % d) / ("s%d" % (d % 3))
        sub.mkdir(parents=True)
        for k in range(150):
            name = ("f%04d.bin" % k) if k % 37 else ("odd name %d: [x]" % k)  # quoted scalars in the middle of a range
            (sub / name).write_bytes(b"%d/%d" % (d, k) if k % 11 else b"")
            n += 1
        if d % 7 == 0:
            os.symlink("f0001.bin", str(sub / "ln"))
    tar = tmp_path / "data.tar.gz"
    tar.write_bytes(b"archive")
    want = oracle.hashes_yaml(str(b), str(tar))
    recs = _lib.walk(str(b))
    assert len(recs) > 9000 and sum(1 for r in recs if r["is_regular"]) == n
    digs = [hashlib.sha512(open(r["path"], "rb").read()).digest() for r in recs if r["is_regular"]]
    got = _lib.emit_yaml(str(b), hashlib.sha512(b"archive").digest(), digs)
    assert got == want
