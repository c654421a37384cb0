"""The flow-update operator's schedule, checked on the CPU.

csrc/update_op.hip and csrc/conv_mfma.hip are compiled host-only and linked with tests/host/operator_trace.cpp, which stands
in for the HIP runtime and prints what it is asked to do (see that file).  Both sections are compared, line by line, with
tests/golden/operator_trace_parent.txt - recorded by tests/golden/make_golden_operator_trace_parent.py from the commit
before the sequencer was rewritten on named descriptors:

    calls     every convolution the sequencer asks for, operand by operand;
    launches  every kernel, grid, block, LDS size and stream the dispatcher makes of them, events and memsets in order.

What stays for the GPU suites: the copy of a descriptor into the kernels' argument block and the translation of the
positional C entry points into a descriptor (tests/test_gpu_conv_epilogues.py, test_gpu_parity.py).
"""

import difflib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vipe_amd", "csrc")
TRACER = os.path.join(ROOT, "tests", "host", "operator_trace.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "operator_trace_parent.txt")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_FLAGS = ["-O1", "-std=c++17", "--offload-arch=gfx950", "--cuda-host-only", "-fPIC", "-ffp-contract=off"]


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, "%s\n%s\n%s" % (" ".join(cmd), r.stdout, r.stderr)
    return r.stdout


def trace(csrc, work, calls_switch="1", extra_flags=()):
    """Builds both tracer programs against the sources in `csrc` and returns the text of the two sections.
    `calls_switch`: TRACE_CALLS of the "calls" program (2: a tree whose sequencer still calls vipe_conv2d_fused);
    `extra_flags`: added to every compile and link (a sanitizer)."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))
    cxx = os.path.join(rocm, "llvm", "bin", "clang++")
    cxx = cxx if os.path.exists(cxx) else shutil.which("c++")
    objs = {}
    for name in ("update_op", "conv_mfma"):
        objs[name] = os.path.join(work, name + ".host.o")
        _run([HIPCC] + HOST_FLAGS + list(extra_flags) + ["-c", os.path.join(csrc, name + ".hip"), "-o", objs[name]])
    out = []
    for section, switch, linked in (("launches", None, ["update_op", "conv_mfma"]), ("calls", calls_switch, ["update_op"])):
        exe = os.path.join(work, "operator_trace_" + section)
        link = [objs[n] for n in linked]
        # a host-only object still names the device code it would carry
        fatbins = sorted(set(re.findall(r"__hip_fatbin_\w+", _run(["nm", "-u"] + link))))
        _run([cxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include")] + list(extra_flags) +
             (["-DTRACE_CALLS=" + switch] if switch else []) + [TRACER] + link +
             ["-Wl,--defsym=%s=0" % f for f in fatbins] + ["-lpthread", "-o", exe])
        out.append("#### %s\n%s" % (section, _run([exe])))
    return "".join(out)


def configurations(text):
    """-> list of (title, lines) per '== ' block (the section headers are blocks of their own)"""
    blocks = []
    for line in text.splitlines():
        if line.startswith(("== ", "#### ")) or not blocks:
            blocks.append((line, []))
        blocks[-1][1].append(line)
    return blocks


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc to compile the sequencer host-only")
def test_operator_trace_matches_parent(tmp_path):
    got, want = configurations(trace(CSRC, str(tmp_path))), configurations(open(GOLDEN).read())
    for (title, g), (_, w) in zip(got, want):
        if g != w:
            pytest.fail("first differing configuration: %s\n%s" % (title, "\n".join(difflib.unified_diff(w, g, "parent", "now", lineterm=""))))
    assert [t for t, _ in got] == [t for t, _ in want]
