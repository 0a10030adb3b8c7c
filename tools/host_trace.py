#!/usr/bin/env python3
"""Does the receiver batch's host code issue the same HIP calls as at an earlier revision?  Builds a stand-alone program from
audiosdr_amd/csrc/asdr_host.cpp at <rev> and from the working tree -- each with a plain host compiler against the recording stubs
(tools/host_trace_stub.cpp) and the scenario driver (tools/host_trace_driver.cpp) of the working tree -- runs every scenario of the
driver in both and compares the traces line by line: every HIP call and every kernel launch with its stream, its events, its
addresses and the whole UpdateArgs.  A refactor of the device-call dispatcher that means to move no call is checked
with this, without a GPU.

  python tools/host_trace.py [<rev>] [--sanitize] [--only <scenario> ...] [--keep <dir>]

<rev> defaults to HEAD~1.  --sanitize builds both programs with -fsanitize=address,undefined (the programs are ordinary host
executables).  --keep leaves the two programs and the traces in <dir>.  Exit status 1 if any scenario differs or fails; nothing in
the checkout changes.  What the trace cannot see: reads of the environment (getenv)."""
import argparse
import difflib
import io
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TOOLS = os.path.join(ROOT, "tools")
CSRC_REL = os.path.join("audiosdr_amd", "csrc")


def toolchain():
    """(host compiler, ROCm include directory), or None when either is missing."""
    cxx = next((c for c in (os.environ.get("CXX"), "g++", "c++", "clang++") if c and shutil.which(c)), None)
    roots = [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    hipcc = shutil.which(os.environ.get("HIPCC") or "hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    inc = next((os.path.join(r, "include") for r in roots if r and os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h"))), None)
    return (cxx, inc) if cxx and inc else None


def build(tree, out, sanitize=False):
    """The trace program of `tree`'s asdr_host.cpp (stubs and driver: the working tree's)."""
    cxx, inc = toolchain()
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-w", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + inc,
           "-I" + os.path.join(tree, "include"), "-I" + os.path.join(tree, CSRC_REL)]
    if sanitize:
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    cmd += [os.path.join(tree, CSRC_REL, "asdr_host.cpp"), os.path.join(TOOLS, "host_trace_stub.cpp"), os.path.join(TOOLS, "host_trace_driver.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("the trace program of %s does not build:\n%s" % (tree, r.stderr[-3000:]))
    return out


def scenarios(prog):
    return subprocess.run([prog, "--list"], capture_output=True, text=True, check=True).stdout.split()


def run(prog, name):
    """The trace of one scenario, as lines."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ASDR_")}   # the switches are the scenario's own
    r = subprocess.run([prog, name], capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0:
        raise RuntimeError("scenario %s of %s ended with status %d:\n%s" % (name, prog, r.returncode, r.stderr[-3000:]))
    return r.stdout.splitlines()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--only", nargs="+")
    ap.add_argument("--keep")
    args = ap.parse_args()
    if toolchain() is None:
        sys.exit("no host compiler, or no ROCm headers (ROCM_PATH)")
    work = args.keep or tempfile.mkdtemp(prefix="host_trace_")
    os.makedirs(work, exist_ok=True)
    bad = 0
    try:
        old = os.path.join(work, "rev")
        shutil.rmtree(old, ignore_errors=True)
        os.makedirs(old)
        tar = subprocess.run(["git", "archive", args.rev, CSRC_REL, "include"], cwd=ROOT, capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old)
        p_old = build(old, os.path.join(work, "host_trace_rev"), args.sanitize)
        p_new = build(ROOT, os.path.join(work, "host_trace_tree"), args.sanitize)
        for name in args.only or scenarios(p_new):
            try:
                a, c = run(p_old, name), run(p_new, name)
            except RuntimeError as e:
                print("%-24s FAILED\n%s" % (name, e))
                bad += 1
                continue
            if args.keep:
                for tag, lines in (("rev", a), ("tree", c)):
                    with open(os.path.join(work, "%s.%s.trace" % (name, tag)), "w") as f:
                        f.write("\n".join(lines) + "\n")
            launches = sum(1 for line in c if line.startswith("asdr_launch_"))
            print("%-24s %s" % (name, "identical (%d lines, %d launches)" % (len(c), launches) if a == c else "DIFFERS"))
            if a != c:
                bad += 1
                for d in list(difflib.unified_diff(a, c, "rev", "tree", n=1, lineterm=""))[:24]:
                    print("    " + d[:300])
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)
    print("asdr_host.cpp: %s" % ("every scenario identical to %s" % args.rev if not bad else "%d scenario(s) differ from %s" % (bad, args.rev)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
