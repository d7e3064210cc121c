"""bench.py on the GPU, on the small BASELINE config 1 tree (101 x 64 KiB): a plain run times `value` and nothing more, and
--full adds the roofline pass, the parity checks, the end_to_end leg and cpu_baseline.  The dumped digests are checked
against hashlib over the synthetic bytes the benchmark wrote (oracle.fill_synthetic: the same generator)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = [pytest.mark.gpu, pytest.mark.kernels_only("runs bench.py in a child process, which names its own flags")]

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "hbm_resident", "parity", "ceilings", "end_to_end", "cpu_baseline")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C1", "--steps", "2",
                        "--warmup", "1"] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert all(k in line for k in HEADLINE) and line["unit"] == "GiB/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and line["ms_per_step"] > 0 and (line["steps"], line["warmup"]) == (2, 1)
    return line


def test_plain_run_times_value_and_dumps_its_outputs(oracle, tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    assert line["config"]["files"] == 101 and line["config"]["ranks"]["distinct_gpus"] == 1
    load = lambda name: np.load(os.path.join(tmp_path, name + ".npy")).astype(np.uint8)  # noqa: E731
    want = [hashlib.sha512(oracle.fill_synthetic(65536, i).tobytes()).digest() for i in range(101)]
    assert [bytes(r) for r in load("file_sha512")] == want[:100]  # d0000/f000000.bin ... f000099.bin, in walk order
    assert bytes(load("archive_sha512")) == want[100]             # the archive stand-in is file index 100
    y = bytes(load("hashes_yaml"))
    assert bytes(load("hashes_yaml_sha512")) == hashlib.sha512(y).digest() and y.count(b"- name: ") == 101  # d0000 and its 100 files


def test_full_run_adds_the_checks_and_legs():
    line = _bench("--full", "--resident-steps", "2")
    assert all(k in line for k in FULL_ONLY), sorted(line)
    assert "byte-identical to the oracle's" in line["parity"]["result"]
    assert line["end_to_end"]["buffers_sharded"]["GiBps"] > 0 and line["cpu_baseline"]["value"] > 0
    assert line["hbm_resident"]["launches_timed"] == 2 and line["roofline"]["achieved"] > 0
