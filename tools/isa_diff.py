#!/usr/bin/env python3
"""Is the gfx950 ISA of a kernel source the same as at an earlier revision?  Compiles the source from a copy of
audiosdr_amd/csrc + include at <rev> and from the working tree (the library's flags, device side only, to assembly), drops
the lines that differ by construction (`__hip_cuid_<hash of the source text>`, `.file`, `.ident`) and compares the listings
kernel by kernel.  A refactor of the chain kernels that means to change no generated code is checked with this, without a GPU.
A kernel on one side only is reported as `removed` or `added`: what it does to the others' listings by construction (the
per-function ordinal in local labels, the column of a comment behind one) is taken out before the comparison.

  python tools/isa_diff.py [<rev>] [--src asdr_kernels.hip] [--variants] [-- extra hipcc flags]

<rev> defaults to HEAD~1.  --variants repeats the comparison for every build that tools/ablate.py and tools/timeline.py
make (-DASDR_TIMELINE, -DASDR_WAVES_PER_EU=2, -DASDR_PIPE_CHUNK=4, -DASDR_NB_ALWAYS_SLOW, each -DASDR_ABLATE=<mask>): those go
through conditions that the default build never compiles.  Exit status 1 if any kernel present on both sides differs; nothing in the checkout changes."""
import argparse
import difflib
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)
from audiosdr_amd import build as b  # noqa: E402

CSRC_REL = os.path.join("audiosdr_amd", "csrc")
DROP = ("__hip_cuid_", ".file", ".ident")
ORDINAL = re.compile(r"(LBB|\bBB|Lfunc_begin|Lfunc_end|LJTI|Ltmp)\d+")   # numbered per function in the order of the file: BB6_2, Lfunc_end6
HEADER = re.compile(r"\s*\.(text|section|protected|globl|weak|hidden|p2align)\b")   # what stands between a function's end and the next one's .type


def listing(tree, src, extra):
    """the split() assembly of `src` compiled in `tree`"""
    flags = [f for f in b.FLAGS if f not in ("-shared", "-fPIC")]
    cmd = [b.hipcc(), "--offload-arch=" + b.ARCH] + flags + list(extra) + ["--cuda-device-only", "-S", src, "-o", "-"]
    out = subprocess.run(cmd, cwd=os.path.join(tree, CSRC_REL), capture_output=True, text=True)
    if out.returncode != 0:
        sys.exit("%s in %s does not compile:\n%s" % (src, tree, out.stderr[-3000:]))
    return split(out.stdout)


def split(asm):
    """{symbol: [lines]} of an assembly listing: one entry per function or kernel, "(other)" for what precedes the first, "(metadata)"
    for the frame of the code-object notes at the end and "(metadata) <kernel>" for a kernel's entry in them."""
    parts, cur = {}, "(other)"
    for line in asm.splitlines():
        if any(d in line for d in DROP):
            continue
        line = re.sub(r"\s+;", " ;", ORDINAL.sub(r"\1#", line))
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            prev, cur = parts.get(cur, []), m.group(1)
            cut = len(prev)
            while cut and HEADER.match(prev[cut - 1]):   # this function's own header lines
                cut -= 1
            parts[cur] = prev[cut:]
            del prev[cut:]
        elif line.strip() == ".amdgpu_metadata" or (cur.startswith("(metadata)") and not line.startswith("    ")):
            cur = "(metadata)"   # the notes' frame; a kernel's entry goes under the kernel's name
            if line.startswith("  - ."):
                cur = "(metadata) entry"
                parts.pop(cur, None)
        elif cur == "(metadata) entry" and line.startswith("    .name:"):
            name = "(metadata) " + line.split()[1]
            parts[name] = parts.pop(cur)
            cur = name
        parts.setdefault(cur, []).append(line)
    return parts


def compare(old, new, label):
    bad = 0
    for name in sorted(set(old) | set(new)):
        a, c = old.get(name), new.get(name)
        state = "removed" if c is None else "added" if a is None else "identical (%d lines)" % len(a) if a == c else "DIFFERS"
        if name.startswith("(metadata) ") and state != "DIFFERS":
            continue   # (a kernel's entry in the notes is worth a line only where it differs on both sides)
        print("%-28s %-44s %s" % (label, name, state))
        if state == "DIFFERS":
            bad += 1
            for d in list(difflib.unified_diff(a, c, "rev", "tree", n=1, lineterm=""))[:24]:
                print("    " + d)
    return bad


def main():
    argv, extra = sys.argv[1:], []
    if "--" in argv:
        extra = argv[argv.index("--") + 1:]
        argv = argv[:argv.index("--")]
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("--src", default="asdr_kernels.hip")
    ap.add_argument("--variants", action="store_true")
    args = ap.parse_args(argv)
    sets = [extra]
    if args.variants:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from ablate import EXTRA, VARIANTS
        sets += [extra + ["-DASDR_TIMELINE"]] + [extra + f for f in EXTRA.values()]
        sets += [extra + ["-DASDR_ABLATE=%d" % m] for m in VARIANTS.values()]
    with tempfile.TemporaryDirectory() as old:
        tar = subprocess.run(["git", "archive", args.rev, CSRC_REL, "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1, 2 * len(sets))) as pool:
            jobs = [(pool.submit(listing, old, args.src, s), pool.submit(listing, ROOT, args.src, s)) for s in sets]
            bad = sum(compare(o.result(), n.result(), " ".join(s) or "(default)") for (o, n), s in zip(jobs, sets))
    print("%s: %s" % (args.src, "every kernel on both sides identical to %s" % args.rev if not bad else "%d listing(s) differ from %s" % (bad, args.rev)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
