"""Where the suite and the tools compile host code: the tests/*_host_harness.cpp models as shared objects for ctypes, and
stand-alone programs (the fake-allocator harnesses, the -D..._MAIN builds, the sanitizer mains).  The only place under
tests/ and tools/ that starts a compiler or sets a sanitizer's environment, and the only statement of what a clean
sanitizer run is (run_sanitized).  Sanitizers run in programs of their own, started directly: nothing here loads one's
runtime into python.

Each build is kept for the life of the process under (sources, flags, defines), in one temporary directory that is
removed at exit; compiles run one at a time.  Each harness's prototypes are declared once, in one memoised load_*()
function in the module of the harness's first user (test_f3_host.load_f3, bz2_check_cases.load_harness, ...)."""
import atexit
import ctypes
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "snappy_amd", "csrc")
# the fake-allocator harnesses read the runtime's headers for their types alone
RUNTIME_HEADERS = ("-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"))
STRICT = ("-Wall", "-Wextra", "-Werror")
SANITIZER_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"}

_built = {}  # (sources, flags, defines) -> path of what they built
_dir = None


def _path(source):
    """A source by its path from the repository's root ("tests/asan_bcj.cpp"), or absolute (a test's own tmp_path)."""
    return os.path.join(ROOT, str(source))


def _build(sources, flags, defines, suffix=""):
    global _dir
    key = (tuple(_path(s) for s in sources), tuple(flags), tuple(defines))
    if key not in _built:
        if _dir is None:
            _dir = tempfile.mkdtemp(prefix="hostbuild-")
            atexit.register(shutil.rmtree, _dir, ignore_errors=True)
        stem = os.path.splitext(os.path.basename(key[0][0]))[0]
        out = os.path.join(_dir, "%s-%d%s" % (stem, len(_built), suffix))
        subprocess.check_call(["g++", "-std=c++17", *key[1], *("-D" + d for d in key[2]), "-o", out, *key[0], "-pthread"])
        _built[key] = out
    return _built[key]


def shared(source, opt="-O2"):
    """A harness as a shared object, loaded.  opt: tools/sha256_bench.py times host SHA-256 at -O3."""
    return ctypes.CDLL(_build([source], (opt, "-shared", "-fPIC"), ()))


def program(sources, flags=("-O2",), defines=()):
    """A host program from sources, flags and defines; returns its path."""
    return _build(sources, flags, defines)


def sanitized(sources, sanitize="address,undefined", flags=(), defines=()):
    """The same with the sanitizers on: address,undefined, or thread for tests/tsan_host.cpp."""
    recover = () if sanitize == "thread" else ("-fno-sanitize-recover=all",)
    return _build(sources, ("-O1", "-g", "-fsanitize=" + sanitize, *recover, *flags), defines)


def run_sanitized(exe, args=(), sanitize="address,undefined", timeout=600):
    """Runs a sanitized program and asserts a clean run: exit status 0, and no report on stderr.  Returns the completed
    process (text), for the caller to check stdout."""
    def run(cmd):
        return subprocess.run([*cmd, exe, *map(str, args)], env=dict(os.environ, **SANITIZER_ENV), capture_output=True, text=True, timeout=timeout)
    r = run([])
    if sanitize == "thread" and r.returncode != 0 and "unexpected memory mapping" in r.stderr:  # the sanitizer runtime against this kernel's ASLR
        r = run(["setarch", "x86_64", "-R"])
        if r.returncode != 0 and "ThreadSanitizer: data race" not in r.stderr and "tsan driver" not in r.stdout and "unexpected memory mapping" in r.stderr:
            import pytest
            pytest.skip("ThreadSanitizer cannot map its shadow on this kernel")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert sanitize != "thread" or "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    return r
