#!/usr/bin/env python3
"""Compare the kernels of two device-assembly files, kernel by kernel.

    hipcc <the FLAGS of csrc/build.py> -x hip -S --cuda-device-only csrc/conv_bf16.hip -o NEW.s      (and the same at the parent commit)
    tools/isa_diff.py PARENT.s NEW.s [--rename REGEX=REPL ...]

Kernels are paired by demangled name, after the renames have been applied to the names of PARENT.s (re.sub; for a kernel that
changed its name or gained template arguments).  Per kernel: whether the two instruction streams are equal -- instructions and labels
only, local labels numbered in order of appearance, no comments, no directives -- and the figures of both kernel descriptors:
VGPRs / AGPR offset / SGPRs / scratch bytes / static LDS bytes.  The streams are compared whole; nothing is searched for in them.
Exit status: 1 when a kernel of either file has no partner, else 0 (a kernel that differs is reported, not an error: the caller's bar
says what may differ)."""
import argparse
import re
import shutil
import subprocess
import sys

FIGURES = ("next_free_vgpr", "accum_offset", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def kernels(path):
    """{demangled name: (instruction stream, figures)} of every .amdhsa_kernel of the file."""
    lines = open(path).read().splitlines()
    figures, name = {}, None
    for ln in lines:
        t = ln.split()
        if t and t[0] == ".amdhsa_kernel":
            name = t[1]
            figures[name] = {}
        elif t and t[0] == ".end_amdhsa_kernel":
            name = None
        elif name and t and t[0].startswith(".amdhsa_") and t[0][8:] in FIGURES:
            figures[name][t[0][8:]] = int(t[1])
    streams = {}
    for i, ln in enumerate(lines):
        m = re.match(r"(\w+):", ln)
        if not m or m.group(1) not in figures:
            continue
        name, body, labels = m.group(1), [], {}
        for ln2 in lines[i + 1:]:
            if ln2.startswith(".Lfunc_end"):
                break
            code = ln2.split(";")[0].strip()
            if not code or (code.startswith(".") and not code.endswith(":")):
                continue   # comment, blank or directive
            code = re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), ".L%d" % len(labels)), code)
            body.append(" ".join(code.replace(name, "SELF").split()))
        streams[name] = body
    mangled = sorted(figures)
    return {d: (streams.get(n, []), figures[n]) for n, d in zip(mangled, demangle(mangled))}


def fig(f):
    return "/".join(str(f.get(k, "-")) for k in FIGURES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL", help="applied to the kernel names of PARENT.s")
    a = ap.parse_args()
    old, new = kernels(a.parent), kernels(a.new)
    for r in a.rename:
        pat, repl = r.split("=", 1)
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    print(f"# {a.parent} ({len(old)} kernels) vs {a.new} ({len(new)} kernels)")
    print("# stream | figures parent -> new (VGPR/AGPR offset/SGPR/scratch/LDS) | instructions parent -> new | kernel")
    same = moved = 0
    for k in sorted(old.keys() & new.keys()):
        (so, fo), (sn, fn) = old[k], new[k]
        eq = so == sn and fo == fn
        same += eq
        moved += not eq
        word = "equal " if so == sn else "DIFFER"
        print(f"{word} | {fig(fo)} -> {fig(fn)}{'' if fo == fn else ' FIGURES DIFFER'} | {len(so)} -> {len(sn)} | {k}")
    unpaired = [(a.parent, k) for k in sorted(old.keys() - new.keys())] + [(a.new, k) for k in sorted(new.keys() - old.keys())]
    for f, k in unpaired:
        print(f"UNPAIRED in {f}: {k}")
    print(f"# {same} identical (stream and figures), {moved} not, {len(unpaired)} unpaired")
    return 1 if unpaired else 0


if __name__ == "__main__":
    sys.exit(main())
