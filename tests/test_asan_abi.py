"""Host AddressSanitizer + UndefinedBehaviorSanitizer run of the C-ABI argument checking
(SURVEY §5 "Host ASan on the C-ABI shim"), one row per public header.

tests/asan_build.py compiles the library's translation units host-only (`--offload-host-only`:
no device code, so no GPU is needed) with -fsanitize=address,undefined, once for the whole
module, and links each header's stand-alone driver tests/asan/abi_args*.cpp against them and
tests/asan/hip_stubs.cpp (a stand-in HIP runtime whose device operations fail and are counted).
A driver calls every entry of its header with NULL pointers, bad shapes, overflowing sizes and
short workspaces; every bad call must return its negative status (or 0 bytes) with no device
operation and no sanitizer report.  GPU sanitizers are not available on this pool; this covers
the host side only."""
import os
import re
import subprocess
from collections import namedtuple

import pytest

import asan_build
from asan_build import REPO

# driver: tests/asan/<driver>.cpp; header: include/<header>; exports: the _lib list the header's
# declarations must equal (None: not compared); floor: the least number of calls the driver makes;
# n_declared: the header's entry count where it is pinned; asan_extra: further ASAN_OPTIONS
Row = namedtuple("Row", "driver header exports floor n_declared asan_extra", defaults=(None, ""))
ROWS = [
    Row("abi_args", "codec_tcc.h", None, 301, asan_extra=":verify_asan_link_order=0"),   # more than 300 calls
    Row("abi_args_ext", "codec_tcc_ext.h", None, 30),
    Row("abi_args_crc", "codec_tcc_crc.h", "EXPORTS_CRC", 40),
    Row("abi_args_vol", "codec_tcc_vol.h", "EXPORTS_VOL", 200),
    Row("abi_args_gate", "codec_tcc_gate.h", "EXPORTS_GATE", 140),
    Row("abi_args_gvol", "codec_tcc_gvol.h", "EXPORTS_GVOL", 150),
    Row("abi_args_tile", "codec_tcc_tile.h", "EXPORTS_TILE", 140),
    Row("abi_args_roi", "codec_tcc_roi.h", "EXPORTS_ROI", 170),
    Row("abi_args_aead", "codec_tcc_aead.h", "EXPORTS_AEAD", 70, 6),
    Row("abi_args_blind", "codec_tcc_blind.h", "EXPORTS_BLIND", 180, 5),
]
rows = pytest.mark.parametrize("row", ROWS, ids=[r.header[:-2] for r in ROWS])


@rows
def test_c_abi_rejects_bad_arguments_under_asan(row):
    if not os.path.exists(asan_build.HIPCC):
        pytest.skip("hipcc not installed")
    exe = asan_build.link_driver(row.driver + ".cpp")
    env = dict(os.environ,
               ASAN_OPTIONS="detect_leaks=0:halt_on_error=1:abort_on_error=0" + row.asan_extra,
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               HIP_VISIBLE_DEVICES="")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    report = r.stdout + r.stderr
    assert "AddressSanitizer" not in report and "runtime error" not in report, report[-6000:]
    assert r.returncode == 0, report[-6000:]
    m = re.search(rf"{row.driver}: (\d+) calls, 0 failures", r.stdout)
    assert m and int(m.group(1)) >= row.floor, report[-3000:]


@rows
def test_every_header_entry_is_driven(row):
    """The driver calls every function its header declares, and the header declares what
    _lib exports for it."""
    hdr = open(os.path.join(REPO, "include", row.header)).read()
    declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(codec_\w+)\s*\(", hdr, re.M))
    called = set(re.findall(r"\b(codec_\w+)\s*\(", open(os.path.join(asan_build.ASAN_DIR, row.driver + ".cpp")).read()))
    from codec_tcc_amd import _lib
    if row.exports:
        assert declared == set(getattr(_lib, row.exports))
    if row.n_declared:
        assert len(declared) == row.n_declared
    assert declared and declared <= called, sorted(declared - called)
    if row.header == "codec_tcc_aead.h":
        assert _lib.KERNEL_TAGS[47] == "k_chacha20_rows" and _lib.KERNEL_TAGS[51] == "k_aead_release"
        assert "#define CODEC_K_CHACHA20_ROWS 47" in hdr and "#define CODEC_K_AEAD_RELEASE 51" in hdr
        assert _lib.AEAD_CTX_BYTES == 48
