"""ScanFrames (quic_fec_wire.cc) under AddressSanitizer + UBSan on the CPU:
tests/cpp/test_scan_frames.cc, a stand-alone program of the sanitized build
test_cpp_sanitizers.py runs (libquic_amd/build.py SAN_TESTS).  Every body, every
prefix of it and random bytes are walked in heap buffers of exactly their
length.  No GPU."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def binaries():
    from libquic_amd import build as B
    return B.build_cpp_sanitized()


def test_scan_frames_under_sanitizers(binaries):
    exe = os.path.join(ROOT, "tests", "cpp", "build", "san_test_scan_frames")
    assert exe in binaries
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert " 0 failures" in out, out[-2000:]
    assert "Sanitizer" not in out and "runtime error" not in out, out[-4000:]
