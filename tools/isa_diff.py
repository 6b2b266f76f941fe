#!/usr/bin/env python3
"""Compare two device assembly files kernel by kernel.

    hipcc <build flags without -shared> -Iinclude --cuda-device-only -S \\
          codec_tcc_amd/csrc/codec_pee.hip -o a.s        # once per tree
    python tools/isa_diff.py a.s b.s [--quiet] [--by-template]

For every kernel symbol (`.amdhsa_kernel NAME`) of either file the report gives: on which
side it exists; the resource numbers (VGPR, AGPR, SGPR, LDS bytes, scratch bytes, occupancy,
code bytes, from the `; Kernel info:` comments) and whether every `.amdhsa_*` directive is
equal; and whether the instruction text is equal once comments are stripped and local labels
(`.LBB3_7`, which carry the function's index in the file) are renumbered in order of
appearance.  Whole texts are compared; which instructions occur is not looked at.

What lies outside the kernels is compared too, so that "identical" means the code object and
not only its kernel bodies: each kernel's record in `.amdgpu_metadata` (its argument list among
others) goes with the kernel's resources, and everything else -- device functions that were not
inlined, `__device__` globals, LDS symbols, the `.set` lines -- is compared as a bag of lines,
labels blanked, since the emission order may move.  The `__hip_cuid_<hash>` lines, which hash
the source path, are left out.

--by-template pairs the kernels by name and template arguments and leaves the parameter list
out of the symbol (`_Z10k_pee_scanItLb1ELb0EE` of `_Z10k_pee_scanItLb1ELb0EEvPKT_...`; an empty
trailing template-argument pack, `J` `E`, is dropped from it).  A template that gains a trailing
pack renames every instantiation, the ones with an empty pack too, and the question is then
whether those kept their resources, argument list and text: the lines that carry the symbol
itself are left out of the comparison, everything else is compared as usual.  Symbols the
pattern does not fit, or that would collide, keep their full name.

Exit status 0 when both files hold the same kernels with equal resources and text and the rest
is equal, else 1.
A refactor that must not touch device code is checked with it (profiles/r11/); so is "what
did this change cost in registers" (the hand-made profiles/r08/kernel_resources.txt and
profiles/r10/gate_isa.txt are of this kind).
"""
from __future__ import annotations

import collections
import re
import sys

INFO_KEYS = [("NumVgprs", "vgpr"), ("NumAgprs", "agpr"), ("TotalNumSgprs", "sgpr"), ("LDSByteSize", "lds"),
             ("ScratchSize", "scratch"), ("Occupancy", "occ"), ("codeLenInByte", "bytes")]
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def parse(path: str):
    """({kernel symbol: {"text": [normalised lines], "amdhsa": [directives], "info": {key: int},
    "meta": [its metadata record]}}, Counter of the lines outside kernels and metadata records)"""
    with open(path) as f:
        lines = f.read().split("\n")
    used = [False] * len(lines)
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    start = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([^\s:;]+):", ln)   # a label in column 0
        if m:
            start.setdefault(m.group(1), i)
    out = {}
    for name in names:
        i0 = i = start[name] + 1
        text, amdhsa, info = [], [], {}
        labels: dict = {}
        in_desc = False
        while not lines[i].startswith(".Lfunc_end"):
            ln = lines[i].split(";", 1)[0].strip()
            i += 1
            if not ln:
                continue
            if ln.startswith(".amdhsa_kernel"):
                in_desc = True
            elif ln.startswith(".end_amdhsa_kernel"):
                in_desc = False
            elif in_desc:
                amdhsa.append(" ".join(ln.split()))
            else:
                text.append(LABEL.sub(lambda m: labels.setdefault(m.group(0), f".L{len(labels)}"), " ".join(ln.split())))
        used[i0:i] = [True] * (i - i0)
        while not lines[i].startswith("; Kernel info:"):
            i += 1
        while lines[i].startswith(";"):
            m = re.match(r";\s*([A-Za-z]+)\s*[:=]\s*(\d+)", lines[i])
            if m:
                info[m.group(1)] = int(m.group(2))
            i += 1
        out[name] = {"text": text, "amdhsa": amdhsa, "info": info, "meta": []}
    # .amdgpu_metadata: one record per kernel, from "  - " at indent 2 to the next one
    if "amdhsa.kernels:" in lines:
        i = lines.index("amdhsa.kernels:") + 1
        while lines[i].startswith("  "):
            j = i + 1
            while lines[j].startswith("   "):
                j += 1
            rec = lines[i:j]
            name = next(ln.split()[1] for ln in rec if ln.strip().startswith(".name:"))
            if name in out:
                out[name]["meta"] = rec
                used[i:j] = [True] * (j - i)
            i = j
    rest = collections.Counter()
    for ln, u in zip(lines, used):
        ln = " ".join(ln.split(";", 1)[0].split())
        if ln and not u and "__hip_cuid_" not in ln:
            rest[LABEL.sub(".L", ln)] += 1
    return out, rest


TEMPLATE_KEY = re.compile(r"_Z\d+[A-Za-z_][A-Za-z_0-9]*?I(?:[a-z]|L[a-z]\d+E|JE)+E(?=v)")


def by_template(kernels: dict) -> dict:
    """The kernels keyed by name and template arguments where that is unambiguous."""
    keys = {}
    for name in kernels:
        m = TEMPLATE_KEY.match(name)
        keys[name] = m.group(0).replace("JE", "") if m else name
    count = collections.Counter(keys.values())
    out = {}
    for name, k in kernels.items():
        out[keys[name] if count[keys[name]] == 1 else name] = dict(
            k, **{part: [ln for ln in k[part] if name not in ln] for part in ("meta", "text", "amdhsa")})
    return out


def numbers(k: dict) -> str:
    return " ".join(f"{short}={k['info'].get(key, '?')}" for key, short in INFO_KEYS)


def main(argv) -> int:
    quiet = "--quiet" in argv
    paths = [a for a in argv if not a.startswith("--")]
    if len(paths) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    (a, rest_a), (b, rest_b) = parse(paths[0]), parse(paths[1])
    if "--by-template" in argv:
        a, b = by_template(a), by_template(b)
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    res_diff = text_diff = 0
    print(f"# A = {paths[0]}: {len(a)} kernels; B = {paths[1]}: {len(b)} kernels")
    print("# per kernel: resources (= equal, ! differ)  text (= equal, ! differ)  symbol  numbers")
    for name in only_a:
        print(f"A-only    {name}  {numbers(a[name])}")
    for name in only_b:
        print(f"B-only    {name}  {numbers(b[name])}")
    for name in sorted(set(a) & set(b)):
        ka, kb = a[name], b[name]
        res_eq = ka["amdhsa"] == kb["amdhsa"] and ka["info"] == kb["info"] and ka["meta"] == kb["meta"]
        text_eq = ka["text"] == kb["text"]
        res_diff += not res_eq
        text_diff += not text_eq
        if quiet and res_eq and text_eq:
            continue
        line = f"res{'=' if res_eq else '!'} text{'=' if text_eq else '!'}  {name}  {numbers(ka)}"
        if not res_eq:
            line += f"  ->  {numbers(kb)}"
        print(line)
    rest_diff = sorted(((rest_a - rest_b) + (rest_b - rest_a)).items())
    for ln, n in rest_diff[:40]:
        print(f"rest!     {n} x {ln}")
    same = not (only_a or only_b or res_diff or text_diff or rest_diff)
    print(f"# only in A: {len(only_a)}; only in B: {len(only_b)}; common: {len(set(a) & set(b))}; "
          f"resources or metadata differ: {res_diff}; text differs: {text_diff}; "
          f"lines outside the kernels: {sum(rest_a.values())} / {sum(rest_b.values())}, differing: {len(rest_diff)}")
    print("# RESULT: " + ("identical kernels, metadata and remainder" if same else "DIFFERENT"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
