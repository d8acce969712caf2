#!/usr/bin/env python3
"""Are the kernels of two builds the same machine code?  Both builds keep their gfx950 code objects
(`ZK_KEEP_HSACO=<dir> make -C zksnake_amd/csrc ...`); functions are matched by mangled name across ALL code objects of a directory,
so a kernel that moved to another translation unit is compared with itself.  Compared per function: the `llvm-objdump -d` text
without addresses and comments, and for kernels (symbols with a `.kd` descriptor) the register, LDS and scratch figures of the
metadata notes.  Two things that belong to a code object's layout and not to the code are masked: the 32-bit literals of the
`s_add_u32` / `s_addc_u32` pair after an `s_getpc_b64` (the distance to a constant table or a callee), and what fills the gap
behind a function: objdump's `...` marker of zeros, and the run of `s_nop 0` that pads the end of a text section and is listed
with whichever function happens to come last in it.  usage: isa_diff.py <dirA> <dirB>; exit status 1 unless everything is equal."""
import glob
import os
import re
import subprocess
import sys

LLVM = "/opt/rocm/lib/llvm/bin"
FIGURES = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size",
           "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack")


def normalise(lines):
    out, pc = [], set()   # pc: scalar registers that hold a program counter whose offset is still to be added
    for line in lines:
        line = line.split("//")[0].strip()
        if not line or line == "...":
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", line)
        if m:
            pc |= {"s" + m.group(1), "s" + m.group(2)}
        m = re.match(r"(s_addc?_u32) (s\d+), (s\d+), \S+$", line)
        if m and m.group(2) == m.group(3) and m.group(2) in pc:
            pc.discard(m.group(2))
            line = f"{m.group(1)} {m.group(2)}, {m.group(3)}, <pc-relative>"
        out.append(line)
    while out and out[-1] == "s_nop 0":   # no function ends in one: it returns, branches or ends the program
        out.pop()
    return out


def load(directory):
    """{(mangled name, code object): (code object, normalised text, figures or None for a function that is no kernel)}"""
    funcs = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.hsaco"))):
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
        meta = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", path], capture_output=True, text=True, check=True).stdout
        figures = {}
        for rec in re.split(r"\n  - (?=\.)", meta)[1:]:   # one record per kernel; its arguments sit deeper
            top = dict(re.findall(r"^    \.(\w+):\s+(\S+)$", "    " + rec, re.M))
            if top.get("symbol", "").endswith(".kd"):
                figures[top["symbol"][:-3]] = tuple(top.get(k) for k in FIGURES)
        for blk in re.split(r"\n(?=[0-9a-f]+ <)", dis):
            m = re.match(r"[0-9a-f]+ <(.+)>:", blk)
            if m and not m.group(1).endswith(".kd"):
                funcs[(m.group(1), os.path.basename(path))] = (os.path.basename(path), normalise(blk.split("\n")[1:]), figures.get(m.group(1)))
    return funcs


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    except OSError:   # no binutils: the mangled names will do
        out = names
    return {n: re.sub(r"^void |\(.*$", "", d) for n, d in zip(names, out)}


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    # a function is matched with its namesake in the same code object; what is left over (it moved, or it is gone) by name alone
    pairs = [(k[0], a[k], b[k]) for k in sorted(set(a) & set(b))]
    left_a, left_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    for k in left_a:
        twin = next((t for t in left_b if t[0] == k[0]), None)
        if twin:
            left_b.remove(twin)
        pairs.append((k[0], a[k], b[twin] if twin else None))
    pairs += [(k[0], None, b[k]) for k in left_b]
    rows, equal, moved = [], [0, 0], 0   # equal kernels, equal other functions
    for name, fa, fb in sorted(pairs, key=lambda p: p[0]):
        moved += bool(fa and fb and fa[0] != fb[0])
        kernel = (fa or fb)[2] is not None
        if fa and fb and fa[1] == fb[1] and fa[2] == fb[2]:
            equal[0 if kernel else 1] += 1
            continue
        if not fa or not fb:
            if not kernel:   # a helper of the device library that every code object carries its own copy of: nothing to compare
                continue
            what = "only in A" if fa else "only in B"
        else:
            lines = sum(1 for x, y in zip(fa[1], fb[1]) if x != y) + abs(len(fa[1]) - len(fb[1]))
            what = f"differs: {len(fa[1])} -> {len(fb[1])} instructions, {lines} lines"
            what += "".join(f", {k} {x} -> {y}" for k, x, y in zip(FIGURES, fa[2] or (), fb[2] or ()) if x != y)
        rows.append((name, "kernel" if kernel else "function", (fa or fb)[0] if not fb or not fa or fa[0] == fb[0] else f"{fa[0]} -> {fb[0]}", what))
    print(f"A = {sys.argv[1]}: {sum(1 for f in a.values() if f[2])} kernels;  B = {sys.argv[2]}: {sum(1 for f in b.values() if f[2])} kernels")
    print(f"equal: {equal[0]} kernels and {equal[1]} other functions; {moved} matched across two code objects")
    names = demangle([r[0] for r in rows])
    if rows:
        print("| function | kind | code object | result |\n|---|---|---|---|")
    for name, kind, where, what in rows:
        print(f"| `{names[name]}` | {kind} | {where} | {what} |")
    return 1 if rows else 0


if __name__ == "__main__":
    sys.exit(main())
