#!/usr/bin/env python3
"""Per-kernel device-code hashes of some units of build.SRCS, one tree against another (the parent
commit's checkout), so that a review sees which existing kernels a change touched.

Per unit and tree: hipcc <build.FLAGS without -shared> -I include --cuda-device-only
--no-gpu-bundle-output -c unit.hip, then every function symbol of the gfx950 code object's .text
(nm -S), its bytes (llvm-objcopy -O binary --only-section=.text) and their sha256.  Kernels are
matched by demangled name without the parameter list; --same-as OLD=NEW (a substring replacement, repeatable) names template
instantiations that gained a parameter.

    python3 tools/device_code_kernels.py --parent /path/to/parent/checkout [--units codec_blind.hip,codec_aead.hip]
        [--same-as 'k_blind_splice<unsigned short>=k_blind_splice<unsigned short, false>'] [--out profiles/r18/device_code.txt]
"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from codec_tcc_amd import build  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"
ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--units", default="codec_blind.hip,codec_aead.hip")
ap.add_argument("--same-as", action="append", default=[])
ap.add_argument("--out", default="")
args = ap.parse_args()


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(tree, unit, tmp):
    """{demangled function name, without parameters: (bytes, sha256 prefix)} of the unit's device .text in `tree`."""
    co = os.path.join(tmp, "unit.co")
    flags = [f for f in build.FLAGS if f != "-shared"]
    run(build.hipcc(), *flags, f"-I{os.path.join(tree, 'include')}", "--cuda-device-only", "--no-gpu-bundle-output", "-c",
        os.path.join(tree, "codec_tcc_amd", "csrc", unit), "-o", co)
    text = os.path.join(tmp, "text.bin")
    run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.text", co, text)
    base = None
    for ln in run("readelf", "-S", "-W", co).splitlines():
        p = ln.replace("[", " ").replace("]", " ").split()
        if len(p) > 4 and p[1] == ".text":
            base = int(p[3], 16)
    data = open(text, "rb").read()
    out = {}
    for ln in run("nm", "-S", "--defined-only", "-C", co).splitlines():
        p = ln.split(None, 3)
        if len(p) == 4 and p[2] in "TtW":
            addr, size = int(p[0], 16), int(p[1], 16)
            body = data[addr - base:addr - base + size]
            name = p[3][5:] if p[3].startswith("void ") else p[3]
            out[name[:name.index("(")] if "(" in name else name] = (size, hashlib.sha256(body).hexdigest()[:16])
    return out


lines = ["Device code per kernel, the parent commit against this commit (tools/device_code_kernels.py): bytes and the first 16",
         "hex digits of the sha256 of each function's bytes in the gfx950 code object's .text.  `new`: no such function in",
         "the parent; a name in brackets: the parent's instantiation it is compared with.", ""]
for unit in args.units.split(","):
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(os.path.abspath(args.parent), unit, tmp), kernels(HERE, unit, tmp)
    renamed = {}
    for rule in args.same_as:
        a, b = rule.split("=", 1)
        for name in old:
            if a in name and name.replace(a, b) in new and name not in new:
                renamed[name.replace(a, b)] = name
    lines.append(f"{unit}: {len(old)} functions in the parent, {len(new)} in this commit")
    same = changed = added = 0
    for name in sorted(new):
        size, h = new[name]
        was = old.get(name) or old.get(renamed.get(name, ""))
        note = f"  [{renamed[name]}]" if name in renamed and name not in old else ""
        if was is None:
            added += 1
            lines.append(f"  new      {size:7d} {h}                            {name}")
        elif was == (size, h):
            same += 1
            lines.append(f"  same     {size:7d} {h}                            {name}{note}")
        else:
            changed += 1
            lines.append(f"  changed  {size:7d} {h}  (parent {was[0]:7d} {was[1]})  {name}{note}")
    gone = [n for n in old if n not in new and n not in renamed.values()]
    for n in sorted(gone):
        lines.append(f"  gone     {old[n][0]:7d} {old[n][1]}                            {n}")
    lines += [f"  {same} same, {changed} changed, {added} new, {len(gone)} gone", ""]
text = "\n".join(lines)
print(text)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
