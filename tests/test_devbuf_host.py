"""The engine's scratch on the CPU: the owning buffer type (snappy_amd/csrc/devbuf.h) and the groups an engine keeps
(engine_bufs.h), built with g++ against a fake allocator that fails its k-th call (tests/devbuf_host_harness.cpp).  A
buffer's pointer and size always agree, and a group whose ensure() fails at any allocation ends empty.  The GPU side of
the same buffers runs in every -m gpu test."""
import os
import subprocess

import pytest

from conftest import ROOT

HARNESS = os.path.join(ROOT, "tests", "devbuf_host_harness.cpp")
# the runtime's headers, for hipError_t and hipEvent_t alone: the harness is a host program and links none of the runtime
RUNTIME_HEADERS = ["-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")]


def build_harness(exe, *flags):
    """The harness as a host program (g++), with the given flags."""
    subprocess.check_call(["g++", "-std=c++17", *flags, *RUNTIME_HEADERS, "-o", exe, HARNESS])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("devbuf") / "devbuf_host")
    build_harness(exe, "-O1", "-Wall", "-Wextra", "-Werror")
    return exe


def run(exe, case, env=None):
    r = subprocess.run([exe, case], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and ("%s ok" % case) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_failed_reserve_leaves_the_buffer_empty(harness):
    """reserve keeps a buffer that is large enough, frees a smaller one before it allocates, and on failure leaves
    size 0 and no pointer; moves hand the block over, pinned buffers pass their NUMA node on."""
    run(harness, "buf")


def test_every_failing_allocation_empties_its_group(harness):
    """For every group (job twins, hashing, compare, staging slot, DEFLATE, inflate, bzip2) and every k, an ensure()
    whose k-th allocation fails leaves every member empty, from empty and from a group sized for a smaller job."""
    r = run(harness, "groups")
    for g in ("job twins", "hashing", "compare", "staging slot", "deflate", "inflate", "bzip2"):
        assert "  %s: " % g in r.stdout, r.stdout


def test_review_sequence_sizes_every_member(harness):
    """ensure(128 chunks) fails after its first buffer, then ensure(4096) succeeds on the same DEFLATE
    group; every member then holds 4096 chunks' worth.  The same for the inflate and bzip2 groups."""
    run(harness, "review")


def test_devbuf_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "devbuf_asan")
    build_harness(exe, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = run(exe, "all", env=env)
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
