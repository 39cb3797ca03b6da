#!/usr/bin/env python3
"""Compare the device assembly of two builds kernel by kernel.

    hipcc $(HIPFLAGS) --cuda-device-only -S file.hip -o DIR/file.s     # for every file, in both trees
    tools/kernel_asm_diff.py OLD_DIR NEW_DIR

Kernels are matched by mangled name over all .s files of a directory, so a kernel may move between files. For every
kernel the instruction stream (comments dropped, the compiler's local labels renumbered in order of appearance: they
carry the function's index in its file) and the .amdhsa_ resource directives (VGPRs, SGPRs, scratch, LDS, ...) must be
equal. Prints one line per kernel and exits nonzero on any difference or on a kernel present on one side only. It
compares text and knows nothing about particular instructions.
"""
import glob
import os
import re
import sys

LOCAL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def kernels(directory):
    """{mangled name: (instruction lines, resource directive lines, file)} of every kernel in directory/*.s"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = open(path).read().split("\n")
        starts = {}  # label -> line index of "name:"
        for i, ln in enumerate(lines):
            m = re.match(r"([A-Za-z_$][\w$.]*):", ln)  # a global label: "name:", possibly followed by a comment
            if m:
                starts.setdefault(m.group(1), i)
        i = 0
        while i < len(lines):
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
            if not m:
                i += 1
                continue
            name, res = m.group(1), []
            i += 1
            while ".end_amdhsa_kernel" not in lines[i]:
                res.append(" ".join(lines[i].split(";")[0].split()))
                i += 1
            body, labels = [], {}
            for ln in lines[starts[name] + 1:]:
                if re.match(r"\.Lfunc_end\d+:", ln):
                    break
                ln = " ".join(ln.split(";")[0].split())
                if ln and not ln.startswith((".amdhsa_", ".end_amdhsa_")):  # the directives are compared on their own
                    body.append(LOCAL.sub(lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), ln))
            if name in out:
                sys.exit("kernel defined twice in %s: %s" % (directory, name))
            out[name] = (body, [r for r in res if r], os.path.basename(path))
    return out


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            verdict = "MISSING: only in " + (sys.argv[1] if name in old else sys.argv[2])
        else:
            (b0, r0, f0), (b1, r1, f1) = old[name], new[name]
            diffs = []
            if b0 != b1:
                first = next((k for k, (x, y) in enumerate(zip(b0, b1)) if x != y), min(len(b0), len(b1)))
                diffs.append("body (%d vs %d lines, first difference at %d)" % (len(b0), len(b1), first))
            diffs += ["%s -> %s" % (x, y) for x, y in zip(r0, r1) if x != y]
            if len(r0) != len(r1):
                diffs.append("resource directives (%d vs %d)" % (len(r0), len(r1)))
            verdict = "DIFFERS: " + "; ".join(diffs) if diffs else "equal"
            verdict += "  [%s%s, %d lines]" % (f1, "" if f0 == f1 else " <- " + f0, len(b1))
        bad += not verdict.startswith("equal")
        print("%s  %s" % (name, verdict))
    n = len(set(old) | set(new))
    print("%d kernels compared, %d equal, %d not" % (n, n - bad, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
