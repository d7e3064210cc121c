"""The engine's HIP events and streams on the CPU: the owning handles, the ledger of timed spans and the stage timer of
snappy_amd/csrc/gpu_handles.h, built with g++ against fake hooks that record every live handle and fail their k-th
creation (tests/gpu_handles_host_harness.cpp).  Every handle created is destroyed exactly once, a caller's stream never;
the ledger's handles outlive its growth, and a second call of the same shape creates none.  The GPU side of the same
types runs in every -m gpu test (tests/test_gpu_timing_fields.py holds the stats they feed)."""
import subprocess

import pytest

import hostbuild

HARNESS = "tests/gpu_handles_host_harness.cpp"


@pytest.fixture(scope="module")
def harness():
    """The harness as a host program: the runtime's headers for its types alone, none of the runtime linked."""
    return hostbuild.program([HARNESS], ("-O1", *hostbuild.STRICT, *hostbuild.RUNTIME_HEADERS))


def run(exe, case, sanitized=False):
    r = hostbuild.run_sanitized(exe, [case]) if sanitized else subprocess.run([exe, case], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and ("%s ok" % case) in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r


def test_every_handle_is_destroyed_once_and_an_adopted_stream_never(harness):
    """Destructor, reset, move construction, move assignment onto a full handle and self-move each leave exactly the
    handles that are still owned; ensure on a full handle creates nothing; a failed creation leaves the handle empty; a
    stream created with a priority gets it, one without gets the runtime's default."""
    run(harness, "handles")


def test_ledger_growth_reuse_failure_and_visiting(harness):
    """1 000 takes leave the first span's handles live and unchanged; after clear() 1 000 more create nothing; a failure
    at each creation of 8 takes leaves whole pairs and used() at what succeeded; the visit gives kinds in take order and
    the sum by kind of a mixed sequence is right, with times the test supplies."""
    run(harness, "ledger")


def test_stage_clock_disabled_creates_nothing_and_a_failed_enable_leaves_none(harness):
    """Disabled, a StageClock owns no event and its marks succeed without recording; a failure at each of its creations
    leaves none behind; enabled, mark(i) records event i and ms(i) reads events i and i + 1."""
    run(harness, "clock")


def test_gpu_handles_under_asan_and_ubsan():
    run(hostbuild.sanitized([HARNESS], flags=hostbuild.RUNTIME_HEADERS), "all", sanitized=True)
