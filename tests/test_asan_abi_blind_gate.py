"""Host AddressSanitizer + UndefinedBehaviorSanitizer run of the argument checking of
include/codec_tcc_blind_gate.h, in the manner of tests/test_asan_abi.py: tests/asan_build.py
compiles the library's translation units host-only with -fsanitize=address,undefined (once per
process, shared with test_asan_abi.py) and links the stand-alone driver
tests/asan/abi_args_blind_gate.cpp against them and the stand-in HIP runtime.  The driver is a
program of its own, run directly as a child process; every bad call must return its negative
status (or 0 bytes) with no device operation and no sanitizer report."""
import os
import re
import subprocess

import pytest

import asan_build
from asan_build import REPO

DRIVER = "abi_args_blind_gate"
HEADER = "codec_tcc_blind_gate.h"
FLOOR = 150   # the least number of calls the driver makes


def test_c_abi_rejects_bad_arguments_under_asan():
    if not os.path.exists(asan_build.HIPCC):
        pytest.skip("hipcc not installed")
    exe = asan_build.link_driver(DRIVER + ".cpp")
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout + r.stderr
    assert "AddressSanitizer" not in report and "runtime error" not in report, report[-6000:]
    assert r.returncode == 0, report[-6000:]
    m = re.search(rf"{DRIVER}: (\d+) calls, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= FLOOR, report[-3000:]


def test_every_header_entry_is_driven():
    """The driver calls every function the header declares, and the header declares what _lib
    exports for it."""
    from codec_tcc_amd import _lib
    hdr = open(os.path.join(REPO, "include", HEADER)).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    called = set(re.findall(r"\b(codec_\w+)\s*\(", open(os.path.join(asan_build.ASAN_DIR, DRIVER + ".cpp")).read()))
    assert declared == set(_lib.EXPORTS_BLIND_GATE) and len(declared) == 3
    assert declared <= called, sorted(declared - called)
