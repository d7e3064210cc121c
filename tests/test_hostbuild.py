"""tests/hostbuild.py itself: every sanitizer test of the suite rests on run_sanitized's idea of a clean run, so that idea
is held against four small programs -- none of which commits a memory error -- and the build cache against itself."""
import os

import pytest

import hostbuild

PROGRAM = '#include <stdio.h>\nint main() {\n    %s\n}\n'
CASES = {
    "clean": 'puts("ok"); return 0;',
    "status": 'return 3;',
    "ubsan": 'fputs("x.cpp:1:1: runtime error: made up\\n", stderr); return 0;',
    "asan": 'fputs("==1==ERROR: AddressSanitizer: made up\\n", stderr); return 0;',
}


def build(tmp_path, case, **kw):
    src = tmp_path / (case + ".cpp")
    src.write_text(PROGRAM % CASES[case])
    return hostbuild.sanitized([src], **kw)


def test_a_clean_run_is_returned_with_its_output(tmp_path):
    r = hostbuild.run_sanitized(build(tmp_path, "clean"))
    assert r.returncode == 0 and r.stdout == "ok\n"


@pytest.mark.parametrize("case", ["status", "ubsan", "asan"])
def test_a_status_or_a_report_on_stderr_is_no_clean_run(tmp_path, case):
    """Exit status 3; status 0 with an UBSan report's line on stderr; status 0 with an ASan report's."""
    exe = build(tmp_path, case)
    with pytest.raises(AssertionError):
        hostbuild.run_sanitized(exe)


def test_builds_are_kept_by_sources_flags_and_defines(tmp_path):
    a = build(tmp_path, "clean")
    made = os.stat(a).st_mtime_ns
    n = len(hostbuild._built)
    assert build(tmp_path, "clean") == a and os.stat(a).st_mtime_ns == made and len(hostbuild._built) == n
    b = build(tmp_path, "clean", defines=["OTHER"])
    assert b != a and os.path.exists(a) and os.path.exists(b) and len(hostbuild._built) == n + 1
