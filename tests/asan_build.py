"""The host-only sanitizer build the C-ABI drivers of tests/asan/ link against (a plain helper
module of tests/test_asan_abi.py, not a pytest plugin).

The library's translation units are compiled host-only (`--offload-host-only`: no device code,
so no GPU is needed) with -fsanitize=address,undefined, once per process, together with
tests/asan/hip_stubs.cpp (a stand-in HIP runtime whose device operations fail and are counted)
and a stub of the build digest.  `link_driver` compiles one stand-alone driver and links it
against those objects with clang++ (no libamdhip64, so no GPU runtime at all); the test runs
the program directly as a child process."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASAN_DIR = os.path.join(REPO, "tests", "asan")
HIPCC = "/opt/rocm/bin/hipcc"
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
SAN = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined"]


def _compile_cmd(src, obj, *extra):
    from codec_tcc_amd import build
    return [HIPCC, "-O1", "-g", "-std=c++17", *extra, "--offload-arch=gfx950", "--offload-host-only", *SAN,
            f"-I{build.INC}", "-c", src, "-o", obj]


@functools.lru_cache(maxsize=None)
def library_objects():
    """(directory, objects): the sanitized host-only objects of every unit in build.SRCS, the HIP
    stubs and the digest stub.  Built on the first call, reused by every later one."""
    from codec_tcc_amd import build
    out = tempfile.mkdtemp(prefix="codec_asan_")
    atexit.register(shutil.rmtree, out, ignore_errors=True)
    objs, jobs = [], []
    for src in build.SRCS:
        obj = os.path.join(out, os.path.basename(src) + ".o")
        print(f"asan_build: compiling unit {os.path.basename(src)}", file=sys.stderr)
        jobs.append(subprocess.Popen(_compile_cmd(src, obj, "-fPIC"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                     text=True))
        objs.append(obj)
    for p in jobs:
        _o, err = p.communicate()
        assert p.returncode == 0, err[-4000:]
    # the host-only objects still name their (absent) code objects: give them empty ones
    nm = subprocess.run(["nm", "-u", *objs], capture_output=True, text=True, check=True).stdout
    fatbins = sorted(set(re.findall(r"\b(__hip_fatbin_[0-9a-f]+)\b", nm)))
    dig = os.path.join(out, "digest.cpp")
    with open(dig, "w") as f:
        f.write('extern "C" const char* codec_build_digest(void) { return "asan-host-build"; }\n' +
                "".join(f'extern "C" {{ char {fb}[64]; }}\n' for fb in fatbins))
    for src in (os.path.join(ASAN_DIR, "hip_stubs.cpp"), dig):
        objs.append(_compile(src, out))
    return out, tuple(objs)


def _compile(src, out):
    obj = os.path.join(out, os.path.basename(src) + ".o")
    r = subprocess.run(_compile_cmd(src, obj), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return obj


def link_driver(driver):
    """Build tests/asan/<driver> (a stand-alone program with its own main) against the library's
    sanitized objects; returns the program's path."""
    out, objs = library_objects()
    exe = os.path.join(out, os.path.splitext(driver)[0])
    r = subprocess.run([CLANGXX, *SAN, *objs, _compile(os.path.join(ASAN_DIR, driver), out), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe
