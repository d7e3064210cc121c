"""bench.py --dump-outputs: the arrays it writes from a hashes.yaml, and the argument checks that run before any GPU work."""
import hashlib
import os
import subprocess
import sys

import numpy as np

from conftest import GOLDEN, ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d, name):
    return np.load(os.path.join(d, name + ".npy"))


def test_dump_outputs_round_trips_the_yaml(tmp_path):
    y = open(os.path.join(GOLDEN, "hashes_simple.yaml"), "rb").read()
    r = bench.dump_outputs(str(tmp_path), y)
    assert r["file_records"] == r["file_records_kept"] == y.count(b"  sha512: ")
    for name in r["files"]:
        assert _load(tmp_path, name[:-4]).dtype in (np.float32, np.float64)
    assert bytes(_load(tmp_path, "hashes_yaml").astype(np.uint8)) == y
    assert bytes(_load(tmp_path, "hashes_yaml_sha512").astype(np.uint8)) == hashlib.sha512(y).digest()
    assert bytes(_load(tmp_path, "archive_sha512").astype(np.uint8)).hex() == y.split(b"\n")[0][16:].decode()
    digests = [bytes(row).hex() for row in _load(tmp_path, "file_sha512").astype(np.uint8)]
    assert digests == [ln[10:].decode() for ln in y.split(b"\n") if ln.startswith(b"  sha512: ")]
    assert list(_load(tmp_path, "file_size")) == [int(ln[8:]) for ln in y.split(b"\n") if ln.startswith(b"  size: ")]


def test_dump_outputs_samples_a_large_yaml_within_the_limit(tmp_path):
    n = bench.DUMP_FILE_ROWS + 1000
    digest = hashlib.sha512(b"").hexdigest().encode()
    y = b"archive-sha512: " + digest + b"\nfiles:\n" + b"".join(
        b"- name: d%04d/f%06d.bin\n  size: %d\n  sha512: %s\n  mode: frw-r--r--\n" % (i // 100, i, i, digest) for i in range(n))
    a = bench.dump_outputs(str(tmp_path / "a"), y)
    b = bench.dump_outputs(str(tmp_path / "b"), y)
    assert a["bytes"] <= bench.DUMP_LIMIT and a["file_records"] == n and a["file_records_kept"] == bench.DUMP_FILE_ROWS
    assert "hashes_yaml_blocks.npy" in a["files"] and len(y) > bench.DUMP_YAML_BYTES
    for name in a["files"]:  # the sample is fixed: two dumps of one output are the same arrays
        assert np.array_equal(_load(tmp_path / "a", name[:-4]), _load(tmp_path / "b", name[:-4]))
    rows = _load(tmp_path / "a", "file_row")
    assert np.array_equal(_load(tmp_path / "a", "file_size"), rows)  # record i has size i
    blocks, index = _load(tmp_path / "a", "hashes_yaml_blocks"), _load(tmp_path / "a", "hashes_yaml_block_index")
    k, at = len(index) // 2, int(index[len(index) // 2]) * bench.DUMP_YAML_BLOCK
    assert bytes(blocks[k].astype(np.uint8)) == y[at:at + bench.DUMP_YAML_BLOCK]


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and r.stdout == b"" and b"--steps must be at least 1" in r.stderr


def test_full_only_options_ask_for_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--legs", "off", "--cpu-seconds", "0"], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 2 and r.stdout == b"" and b"--cpu-seconds / --legs configure what --full adds" in r.stderr


def test_plain_run_is_the_default_and_full_keeps_its_defaults(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse_args()
    assert not a.full and (a.cpu_seconds, a.legs, a.resident_steps) == (20.0, "auto", 12)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse_args()
    assert a.full and (a.cpu_seconds, a.legs, a.resident_steps) == (20.0, "auto", 12)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--legs", "off", "--cpu-seconds", "0", "--resident-steps", "2"])
    a = bench.parse_args()
    assert a.full and (a.cpu_seconds, a.legs, a.resident_steps) == (0.0, "off", 2)
