"""The engine's scratch on the CPU: the owning buffer type (snappy_amd/csrc/devbuf.h) and the groups an engine keeps
(engine_bufs.h), built with g++ against a fake allocator that fails its k-th call (tests/devbuf_host_harness.cpp).  A
buffer's pointer and size always agree, and a group whose ensure() fails at any allocation ends empty.  The GPU side of
the same buffers runs in every -m gpu test."""
import subprocess

import pytest

import hostbuild

HARNESS = "tests/devbuf_host_harness.cpp"


@pytest.fixture(scope="module")
def harness():
    """The harness as a host program: the runtime's headers for hipError_t and hipEvent_t alone, none of the runtime linked."""
    return hostbuild.program([HARNESS], ("-O1", *hostbuild.STRICT, *hostbuild.RUNTIME_HEADERS))


def run(exe, case, sanitized=False):
    r = hostbuild.run_sanitized(exe, [case]) if sanitized else subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
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
    run(hostbuild.sanitized([HARNESS], flags=hostbuild.RUNTIME_HEADERS), "all", sanitized=True)
