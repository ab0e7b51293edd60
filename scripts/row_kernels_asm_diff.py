"""The row kernels' gfx950 code at two commits, kernel by kernel: did a change to the shared headers change what the compiler makes?

    python scripts/row_kernels_asm_diff.py [--parent HEAD] [--markdown]

Compiles hip/sampler.hip, voice.hip, resample.hip, polyphony.hip, biquad.hip, program.hip, sweep.hip, filter_program.hip and stream.hip device-only to assembly with build.py's flags, once from the files of
`--parent` (a git revision, exported into a temporary directory) and once from the working tree, and compares every kernel's
instruction stream (comments and directives dropped, the function's number taken out of its labels) and its VGPR, SGPR, scratch and LDS
figures from the code object's metadata.  A file or a kernel that only the working tree has (at the commit that adds them: the sweeps' families) is listed
as `new` with its figures.  A kernel is `identical`, differs in `operand order` (same length, line by line the same
opcode and the same operands in another order), or `differs`.  Needs hipcc and no GPU.  Exit status 1 if a kernel of the parent is missing."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oalsfxpp_amd import build  # noqa: E402

SOURCES = ["sampler", "voice", "resample", "polyphony", "biquad", "program", "sweep", "filter_program", "stream"]
FIGURES = (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def assembly(tree, out_dir, sources):
    """{source: assembly text} of the tree's files hip/<source>.hip."""
    csrc = os.path.join(tree, "oalsfxpp_amd", "csrc")
    flags = [f for f in build.COMMON if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"), "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(csrc, "hip")]
    procs = {}
    for name in sources:
        if not os.path.exists(os.path.join(csrc, "hip", name + ".hip")):
            continue
        out = os.path.join(out_dir, name + ".s")
        procs[name] = (out, subprocess.Popen([build._hipcc()] + flags + build.DEVICE + ["--cuda-device-only", "-S", os.path.join(csrc, "hip", name + ".hip"), "-o", out]))
    texts = {}
    for name, (out, p) in procs.items():
        if p.wait() != 0:
            sys.exit(f"hipcc failed on {name}.hip in {tree}")
        texts[name] = open(out).read()
    return texts


def demangle(names):
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build._hipcc()))), "llvm", "bin", "llvm-cxxfilt")
    tool = tool if os.path.exists(tool) else "c++filt"
    out = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {n: re.sub(r"^(void )?(oalsfx_hip::)?|\(.*$", "", d) for n, d in zip(names, out)}


def kernels(text):
    """{kernel: (instructions, figures)} of one assembly file."""
    figures = {}
    for entry in re.split(r"\n  - \.", text[text.index("amdhsa.kernels:"):])[1:]:
        entry = "." + entry
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        figures[name] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", entry).group(1)) for k in FIGURES)
    pretty = demangle(sorted(figures))
    found = {}
    for name in figures:
        body = text[text.index(f"\n{name}:") + len(name) + 2:]
        body = body[:re.search(r"\n\.Lfunc_end\d+:", body).start()]
        lines = []
        for line in body.split("\n"):
            line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].strip())
            if line and not (line.startswith(".") and not line.startswith(".LBB_")):
                lines.append(line)
        found[pretty[name]] = (lines, figures[name])
    return found


def instructions(lines):
    return [l for l in lines if not l.endswith(":")]


def verdict(a, b):
    if a == b:
        return "identical"
    if len(a) == len(b) and all(x == y or (x.split(None, 1)[0] == y.split(None, 1)[0] and sorted(re.split(r",\s*", x.split(None, 1)[-1])) == sorted(re.split(r",\s*", y.split(None, 1)[-1])))
                                for x, y in zip(a, b)):
        return f"operand order ({sum(x != y for x, y in zip(a, b))} lines)"
    same_mix = collections.Counter(l.split()[0] for l in instructions(a)) == collections.Counter(l.split()[0] for l in instructions(b))
    return "differs" + (", same opcode histogram" if same_mix else "")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--sources", nargs="+", default=SOURCES, help="hip/<name>.hip files to compare instead of the row kernels', e.g. support_kernels")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        parent = os.path.join(tmp, "parent")
        os.makedirs(parent)
        archive = subprocess.run(["git", "-C", ROOT, "archive", args.parent, "include", "oalsfxpp_amd/csrc"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", parent], input=archive, check=True)
        os.makedirs(os.path.join(tmp, "a"))
        os.makedirs(os.path.join(tmp, "b"))
        before, after = assembly(parent, os.path.join(tmp, "a"), args.sources), assembly(ROOT, os.path.join(tmp, "b"), args.sources)
    status = 0
    if args.markdown:
        print("| kernel | instructions, parent | change | stream | VGPR, SGPR, scratch, LDS parent | change |\n|---|---|---|---|---|---|")
    for name in args.sources:
        old, new = kernels(before[name]) if name in before else {}, kernels(after[name])
        if set(old) - set(new):
            print(f"{name}.hip: kernels missing: {sorted(set(old) - set(new))}")
            status = 1
        for k in sorted(set(new) - set(old)):
            row = (f"`{k}`", "-", len(instructions(new[k][0])), "new", "-", ", ".join(map(str, new[k][1])))
            print(("| " + " | ".join(map(str, row)) + " |") if args.markdown else "  ".join(map(str, row)))
        for k in sorted(set(old) & set(new)):
            (a, fa), (b, fb) = old[k], new[k]
            row = (f"`{k}`", len(instructions(a)), len(instructions(b)), verdict(a, b), ", ".join(map(str, fa)), "same" if fa == fb else ", ".join(map(str, fb)))
            print(("| " + " | ".join(map(str, row)) + " |") if args.markdown else "  ".join(map(str, row)))
    return status


if __name__ == "__main__":
    sys.exit(main())
