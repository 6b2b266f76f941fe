"""Host AddressSanitizer + UndefinedBehaviorSanitizer run of the argument checking of the
entries in include/codec_tcc_blind.h, built the way tests/test_asan_abi_roi.py builds its driver:
the library's translation units host-only with -fsanitize=address,undefined, linked against
tests/asan/hip_stubs.cpp and the stand-alone driver tests/asan/abi_args_blind.cpp, which is run
directly.  Every bad call (NULL pointers, bad shapes, H or W above 65535, T above 64, slices below
192 pixels, out-of-range max_entries / user_words, rows narrower than the side bits, in-place
buffers, short workspaces) must return its negative status with no device operation and no
sanitizer report; every call with good arguments must reach its first device operation."""
import os
import re
import subprocess

import pytest

from test_asan_abi import HIPCC, REPO, SAN

DRIVER = os.path.join(REPO, "tests", "asan", "abi_args_blind.cpp")


@pytest.fixture(scope="module")
def abi_args_blind_binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    from codec_tcc_amd import build
    out = tmp_path_factory.mktemp("asan_blind")
    objs = []
    jobs = []
    for src in build.SRCS:
        obj = str(out / (os.path.basename(src) + ".o"))
        cmd = [HIPCC, "-O1", "-g", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "--offload-host-only", *SAN,
               f"-I{build.INC}", "-c", src, "-o", obj]
        jobs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
        objs.append(obj)
    for p in jobs:
        _o, err = p.communicate()
        assert p.returncode == 0, err[-4000:]
    # the host-only objects still name their (absent) code objects: give them empty ones
    nm = subprocess.run(["nm", "-u", *objs], capture_output=True, text=True, check=True).stdout
    fatbins = sorted(set(re.findall(r"\b(__hip_fatbin_[0-9a-f]+)\b", nm)))
    dig = out / "digest.cpp"
    dig.write_text('extern "C" const char* codec_build_digest(void) { return "asan-host-build"; }\n' +
                   "".join(f'extern "C" {{ char {f}[64]; }}\n' for f in fatbins))
    for src in (DRIVER, os.path.join(REPO, "tests", "asan", "hip_stubs.cpp"), str(dig)):
        obj = str(out / (os.path.basename(src) + ".o"))
        r = subprocess.run([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "--offload-host-only", *SAN,
                            f"-I{build.INC}", "-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
        objs.append(obj)
    exe = str(out / "abi_args_blind")
    # linked with clang++ against the stubs only (no libamdhip64, so no GPU runtime at all)
    r = subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", *SAN, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_blind_c_abi_rejects_bad_arguments_under_asan(abi_args_blind_binary):
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([abi_args_blind_binary], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout + r.stderr
    assert "AddressSanitizer" not in report and "runtime error" not in report, report[-6000:]
    assert r.returncode == 0, report[-6000:]
    m = re.search(r"abi_args_blind: (\d+) calls, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 180, report[-3000:]


def test_every_blind_header_entry_is_driven():
    """abi_args_blind.cpp calls every function include/codec_tcc_blind.h declares, and the
    loader's list is exactly the header's."""
    hdr = open(os.path.join(REPO, "include", "codec_tcc_blind.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    called = set(re.findall(r"\b(codec_\w+)\s*\(", open(DRIVER).read()))
    from codec_tcc_amd import _lib
    assert declared == set(_lib.EXPORTS_BLIND) and len(declared) == 5
    assert declared and declared <= called, sorted(declared - called)
