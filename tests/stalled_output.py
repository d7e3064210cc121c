"""A deterministic window into a producer that has no callback: its output is a FIFO.

tar_create_impl (targz.inc) walks and plans the tree, THEN opens the output with O_WRONLY | O_CREAT, then reads the first
byte of the first file.  On a FIFO that open sleeps until somebody opens the other end -- so between "the sizes are taken"
and "the bytes are read" the calling thread sits in open()/openat(), for as long as the test likes.  run_stalled():

    makes the FIFO, runs the call on a thread of its own, waits until that thread is asleep in open/openat (state S in
    /proc/self/task/<tid>/status, the system call's number first in /proc/self/task/<tid>/syscall, in several polls in a row:
    the walk's own opens do not sleep, its waits for walker threads are futex waits), runs the mutation, opens the FIFO for
    reading IN A FINALLY and drains it to its end on a second thread, joins both -- also when the mutation itself
    raised: its exception leaves only after the call has come back (or has been counted as hung).

Every wait has a limit.  A limit reached raises StalledOutputError (an AssertionError: the test fails, it is never skipped)
and sets WEDGED, which the GPU tests look at before they make another call: a call that never came back may still hold
the context.  tests/test_stalled_output.py tests the gate itself on the CPU."""
import os
import platform
import threading
import time

# open / openat by machine (asm/unistd.h); the generic table (aarch64, riscv64) has openat alone
_OPEN_NUMBERS = {"x86_64": (2, 257), "aarch64": (56,), "riscv64": (56,), "ppc64le": (5, 286), "s390x": (5, 288)}
OPEN_NUMBERS = _OPEN_NUMBERS.get(platform.machine(), (257,))

WEDGED = False  # a call outlived its limit: no further GPU call in this process


class StalledOutputError(AssertionError):
    pass


def _task_state(tid):
    """(state letter, number of the system call the task is in or -1) -- (None, -1) if the task is gone."""
    try:
        with open("/proc/self/task/%d/status" % tid) as f:
            state = next((ln.split()[1] for ln in f if ln.startswith("State:")), None)
        with open("/proc/self/task/%d/syscall" % tid) as f:
            first = f.read().split()[0]
        return state, int(first) if first.lstrip("-").isdigit() else -1  # ("running": the task is not in a system call)
    except (FileNotFoundError, ProcessLookupError, StopIteration, IndexError):
        return None, -1


def asleep_in_open(tid):
    state, nr = _task_state(tid)
    return state == "S" and nr in OPEN_NUMBERS


def _unstick(fifo):
    """Lets whoever sleeps in an open of the FIFO go on (a limit was reached: the test fails anyway)."""
    try:
        os.close(os.open(fifo, os.O_RDWR | os.O_NONBLOCK))
    except OSError:
        pass


def run_stalled(fifo, call, mutate, open_limit=30.0, call_limit=120.0, polls=3, interval=0.001):
    """call(): the producer call whose output path is `fifo` (made here; the path must not exist).  mutate(): run while the
    call sleeps in the open of its output.  -> (result, exception, bytes): what call() returned or raised, and everything it
    wrote into the FIFO."""
    global WEDGED
    os.mkfifo(fifo)
    box = {"out": b""}
    started, done = threading.Event(), threading.Event()

    def runner():
        box["tid"] = threading.get_native_id()
        started.set()
        try:
            box["result"] = call()
        except BaseException as e:  # noqa: B902  (handed to the caller)
            box["exc"] = e
        finally:
            done.set()

    def drain():
        try:
            # (non-blocking open: returns at once even if the call never got to its open; a writer asleep in open() is
            # counted as a writer already, so the reads below wait for its bytes)
            fd = os.open(fifo, os.O_RDONLY | os.O_NONBLOCK)
        except OSError as e:
            box["drain_exc"] = e
            return
        try:
            os.set_blocking(fd, True)
            chunks = []
            while True:
                b = os.read(fd, 1 << 20)
                if not b:
                    break
                chunks.append(b)
            box["out"] = b"".join(chunks)
        finally:
            os.close(fd)

    t_call = threading.Thread(target=runner, daemon=True)
    t_drain = threading.Thread(target=drain, daemon=True)
    t_call.start()
    problem = None
    try:
        if not started.wait(open_limit):
            problem = "the call's thread did not start"
        else:
            deadline, seen = time.monotonic() + open_limit, 0
            while seen < polls:
                if done.is_set():
                    problem = "the call ended without sleeping in the open of its output: %r" % (box.get("exc", box.get("result")),)
                    break
                if time.monotonic() > deadline:
                    problem = "the call did not open its output within %.0f s (last seen: %r)" % (open_limit, _task_state(box["tid"]))
                    break
                seen = seen + 1 if asleep_in_open(box["tid"]) else 0
                time.sleep(interval)
            if problem is None:
                box["gate_opened"] = True
                try:
                    mutate()
                except BaseException as e:  # noqa: B902  (raised again below, once the call has been joined)
                    box["mutate_exc"] = e
    finally:
        t_drain.start()  # the reader: whatever happened above, the call is not left asleep in its open
    t_call.join(call_limit)
    t_drain.join(call_limit if not t_call.is_alive() else 1.0)
    if t_call.is_alive() or t_drain.is_alive():
        WEDGED = True
        _unstick(fifo)
        raise StalledOutputError("limit reached: call %s, reader %s%s" % ("still running" if t_call.is_alive() else "ended",
                                 "still running" if t_drain.is_alive() else "ended", "; " + problem if problem else ""))
    if "mutate_exc" in box:
        raise box["mutate_exc"]
    if problem:
        raise StalledOutputError(problem)
    if "drain_exc" in box:
        raise StalledOutputError("the FIFO could not be opened for reading: %r" % (box["drain_exc"],))
    return box.get("result"), box.get("exc"), box["out"]
