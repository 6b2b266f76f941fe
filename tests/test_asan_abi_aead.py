"""Host AddressSanitizer + UndefinedBehaviorSanitizer run of the argument checking of the
entries in include/codec_tcc_aead.h, built the way tests/test_asan_abi_crc.py builds its driver:
the library's translation units host-only with -fsanitize=address,undefined, linked against
tests/asan/hip_stubs.cpp and the stand-alone driver tests/asan/abi_args_aead.cpp, which is run
directly.  Every bad call must return its negative status with no device operation and no
sanitizer report."""
import os
import re
import subprocess

import pytest

from test_asan_abi import HIPCC, REPO, SAN

DRIVER = os.path.join(REPO, "tests", "asan", "abi_args_aead.cpp")


@pytest.fixture(scope="module")
def abi_args_aead_binary(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    from codec_tcc_amd import build
    out = tmp_path_factory.mktemp("asan_aead")
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
    exe = str(out / "abi_args_aead")
    # linked with clang++ against the stubs only (no libamdhip64, so no GPU runtime at all)
    r = subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", *SAN, *objs, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def test_aead_c_abi_rejects_bad_arguments_under_asan(abi_args_aead_binary):
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([abi_args_aead_binary], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout + r.stderr
    assert "AddressSanitizer" not in report and "runtime error" not in report, report[-6000:]
    assert r.returncode == 0, report[-6000:]
    m = re.search(r"abi_args_aead: (\d+) calls, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= 70, report[-3000:]


def test_every_aead_header_entry_is_driven():
    """abi_args_aead.cpp calls every function include/codec_tcc_aead.h declares."""
    hdr = open(os.path.join(REPO, "include", "codec_tcc_aead.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    called = set(re.findall(r"\b(codec_\w+)\s*\(", open(DRIVER).read()))
    from codec_tcc_amd import _lib
    assert declared == set(_lib.EXPORTS_AEAD) and len(declared) == 6
    assert declared and declared <= called, sorted(declared - called)
    assert _lib.KERNEL_TAGS[47] == "k_chacha20_rows" and _lib.KERNEL_TAGS[51] == "k_aead_release"
    assert "#define CODEC_K_CHACHA20_ROWS 47" in hdr and "#define CODEC_K_AEAD_RELEASE 51" in hdr
    assert _lib.AEAD_CTX_BYTES == 48
