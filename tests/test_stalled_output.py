"""The FIFO gate of tests/stalled_output.py, on the CPU, against a stand-in for a producer call: it lists a directory (opens
that do not sleep), waits on a threading.Event (a futex wait, like the walk's wait for its walker threads), and only then
opens the FIFO for writing.  The gate must not open before that open, must open after it, and must fail loudly -- within
its limit -- on a call that never opens its output."""
import os
import threading
import time

import pytest

import stalled_output


def test_gate_opens_after_the_open_and_not_before(tmp_path):
    fifo = str(tmp_path / "out.fifo")
    go = threading.Event()
    marks = {}

    def call():
        for _ in range(50):
            os.listdir(str(tmp_path))
        go.wait(30)                       # asleep, but not in open(): the gate stays shut
        marks["before_open"] = time.monotonic()
        fd = os.open(fifo, os.O_WRONLY)   # sleeps until the helper's reader comes
        marks["after_open"] = time.monotonic()
        try:
            os.write(fd, b"payload" * 1000)
        finally:
            os.close(fd)
        return "done"

    def release():  # the call is held in its futex wait for a while: some hundred polls of the gate see it there
        time.sleep(0.05)
        marks["released"] = time.monotonic()
        go.set()

    def mutate():
        marks["mutated"] = time.monotonic()
        marks["open_returned_before_mutation"] = "after_open" in marks

    threading.Thread(target=release, daemon=True).start()
    t0 = time.monotonic()
    result, exc, out = stalled_output.run_stalled(fifo, call, mutate, open_limit=30, call_limit=30)
    took = time.monotonic() - t0
    assert exc is None and result == "done" and out == b"payload" * 1000
    # no wait of the helper may be ended by its limit instead of its event: the stand-in sleeps 50 ms, the gate needs three
    # polls of a millisecond, the rest is thread start-up -- five seconds is a hundred times that, and a sixth of any limit
    assert took < 5.0, (took, marks)
    assert marks["mutated"] - marks["before_open"] < 2.0 and marks["after_open"] - marks["mutated"] < 2.0, marks
    assert marks["released"] <= marks["before_open"] <= marks["mutated"] <= marks["after_open"], marks
    assert not marks["open_returned_before_mutation"]
    assert not stalled_output.WEDGED


def test_gate_fails_loudly_on_a_call_that_never_opens(tmp_path):
    fifo = str(tmp_path / "out.fifo")
    never = threading.Event()
    mutated = []
    try:
        with pytest.raises(stalled_output.StalledOutputError) as ei:
            stalled_output.run_stalled(fifo, lambda: never.wait(30), lambda: mutated.append(1), open_limit=0.2, call_limit=0.2)
        assert "limit reached" in str(ei.value) and "did not open its output" in str(ei.value)
        assert not mutated and stalled_output.WEDGED
    finally:
        never.set()
        stalled_output.WEDGED = False  # (this process's stand-in, not a GPU call)


def test_gate_reports_a_call_that_ends_before_its_open(tmp_path):
    fifo = str(tmp_path / "out.fifo")

    def call():
        raise OSError(2, "walk failed")

    mutated = []
    with pytest.raises(stalled_output.StalledOutputError) as ei:
        stalled_output.run_stalled(fifo, call, lambda: mutated.append(1), open_limit=5, call_limit=5)
    assert "ended without sleeping in the open" in str(ei.value) and not mutated and not stalled_output.WEDGED


def test_a_mutation_that_raises_leaves_after_the_call_has_been_joined(tmp_path):
    fifo = str(tmp_path / "out.fifo")
    ended = []

    def call():
        fd = os.open(fifo, os.O_WRONLY)
        os.close(fd)
        time.sleep(0.05)  # still at work when the mutation has long raised
        ended.append(time.monotonic())

    def mutate():
        raise ValueError("mutation failed")

    with pytest.raises(ValueError):
        stalled_output.run_stalled(fifo, call, mutate, open_limit=10, call_limit=10)
    assert ended and not stalled_output.WEDGED
