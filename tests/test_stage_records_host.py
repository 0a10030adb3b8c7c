"""The record holder, the settings mirror and the block-row refusals of audiosdr_amd/csrc/asdr_stage_host.h on a CPU, under the address and
undefined-behaviour sanitizers: tests/host_c/stage_records_main.cpp, a stand-alone program with its own main, compares them with plain
loops for a 48-byte and a 704-byte record (fill, rewrite, write with and without a channel list, refused lists that write nothing, read,
apply for one channel and for all).  The HIP functions the header names come from tools/host_trace_stub.cpp, which carries memory
operations out on host memory.  The program is built with the host compiler and run directly; no GPU."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import host_trace  # noqa: E402


def test_stage_records_and_mirror_under_sanitizers(tmp_path):
    tools = host_trace.toolchain()
    if tools is None:
        pytest.fail("no host C++ compiler or no HIP headers")
    cxx, inc = tools
    exe = tmp_path / "stage_records"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I" + inc,
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "audiosdr_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-static-libsan" if "clang" in os.path.basename(cxx) else "-static-libasan",      # the runtime is part of the program
           os.path.join(ROOT, "tests", "host_c", "stage_records_main.cpp"), os.path.join(ROOT, "tools", "host_trace_stub.cpp"), "-o", str(exe)]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout[-500:], run.stderr[-3000:])
    assert run.stdout.rstrip().endswith("stage records ok")
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
