#!/usr/bin/env python3
"""Two device listings of one translation unit, kernel by kernel: tools/isa_diff.py parent.s new.s [name-filter]
(`hipcc --offload-arch=gfx950 <the file's flags> --cuda-device-only -S`; no GPU needed).  One markdown table: per kernel the
compiler's own VGPRs, scratch bytes, LDS bytes and occupancy and the instructions of its body, first listing then second, and a
verdict: "same code" when the two instruction streams are equal text (operands and order included; only the function's number in
its block labels is ignored), else "same vector opcodes" when the histograms of the v_* / global_* / ds_* opcodes are equal --
which says nothing about scalar instructions, order or registers, so the columns that changed are named beside it --, else how
those histograms differ (second minus first).  A kernel of one listing only has one side."""
import collections
import re
import shutil
import subprocess
import sys

LLVM = "/opt/rocm/lib/llvm/bin"
INFO = {"NumVgprs": "vgpr", "ScratchSize": "scratch", "LDSByteSize": "lds", "Occupancy": "occ"}


def demangle(names):
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt", path=LLVM)
    if not filt:
        return {n: n for n in names}
    # (binutils' demangler does not know the bf16 builtin: hand it over as a vendor type of that name)
    out = subprocess.run([filt], input="\n".join(n.replace("DF16b", "u4bf16") for n in names), capture_output=True, text=True).stdout.splitlines()
    out = [re.sub(r"\(anonymous namespace\)::", "", n) for n in out]
    out = [re.sub(r"^void ", "", n) for n in out]
    out = [re.sub(r"\(.*$", "", n).replace("__hip_bfloat16", "bf16").replace("__bf16", "bf16") for n in out]
    return dict(zip(names, out))


def kernels(path):
    """{mangled name: {"vgpr", "scratch", "lds", "occ", "instr", "ops": Counter}} for every function that carries kernel info"""
    found, name, cur = {}, None, None
    for ln in open(path):
        m = re.match(r"(\w+):\s+; @\1\s*$", ln)
        if m:
            name, cur = m.group(1), {"instr": 0, "ops": collections.Counter(), "body": True, "text": []}
            continue
        if cur is None:
            continue
        if cur["body"]:
            m = re.match(r"\t([a-z][a-z0-9_]*)(\s|$)", ln)
            if m:
                cur["instr"] += 1
                cur["text"].append(re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip()))
                if m.group(1).split("_")[0] in ("v", "global", "ds"):
                    cur["ops"][m.group(1)] += 1
            elif ln.startswith("\t.section"):
                cur["body"] = False
            continue
        m = re.match(r"; (\w+): (\d+)", ln)
        if m and m.group(1) in INFO:
            cur[INFO[m.group(1)]] = int(m.group(2))
            if m.group(1) == "Occupancy":
                found[name] = cur
                cur = None
    return found


def main(a, b, flt=""):
    A, B = kernels(a), kernels(b)
    names = demangle(sorted(set(A) | set(B)))                        # a kernel is the same kernel whatever its parameter list
    A, B = {names[m]: k for m, k in A.items()}, {names[m]: k for m, k in B.items()}
    cols = ("vgpr", "scratch", "lds", "occ", "instr")
    print("| kernel | " + " | ".join(f"1: {c}" if i == 0 else c for i, c in enumerate(cols)) + " | "
          + " | ".join(f"2: {c}" if i == 0 else c for i, c in enumerate(cols)) + " | verdict |")
    print("|" + "---|" * (2 * len(cols) + 2))
    details = []
    for n in sorted(set(A) | set(B)):
        if flt and flt not in n:
            continue
        ka, kb = A.get(n), B.get(n)
        side = lambda k: " | ".join(str(k[c]) if k else "-" for c in cols)
        if ka and kb:
            d = {op: kb["ops"][op] - ka["ops"][op] for op in set(ka["ops"]) | set(kb["ops"]) if kb["ops"][op] != ka["ops"][op]}
            moved = [c for c in cols if ka[c] != kb[c]]
            if ka["text"] == kb["text"]:
                note = "same code"
            elif not d:
                note = "same vector opcodes" + (f"; {', '.join(moved)} changed" if moved else "; scalar code or order changed")
            else:
                note = f"differ ({sum(ka['ops'].values())} -> {sum(kb['ops'].values())})"
            if d:
                details.append(f"- `{n}`: " + ", ".join(f"{op} {d[op]:+d}" for op in sorted(d)))
        else:
            note = "only in the second" if kb else "only in the first"
        print(f"| `{n}` | {side(ka)} | {side(kb)} | {note} |")
    if details:
        print("\nPer kernel, the opcodes whose count changed (second minus first):\n")
        print("\n".join(details))


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(*sys.argv[1:4])
