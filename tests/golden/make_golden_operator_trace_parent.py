"""Writes operator_trace_parent.txt: the two sections of tests/host/operator_trace.cpp - every convolution the flow-update
operator's sequencer asks for, and every kernel launch, event and memset the library makes of them - recorded from the
commit BEFORE the sequencer was rewritten on named descriptors (csrc/conv_call.cuh).  No GPU is needed:

    python tests/golden/make_golden_operator_trace_parent.py [--parent 65f5409] [--out tests/golden/operator_trace_parent.txt]

The parent is checked out into a temporary directory; its update_op.hip and conv_mfma.hip are compiled host-only and linked
with THIS tree's tracer.  The parent's sequencer calls the positional vipe_conv2d_fused, so its "calls" program is built
with TRACE_CALLS=2: the tracer intercepts that entry point and maps its arguments onto the canonical form of a descriptor.
tests/test_operator_trace.py compares the current sources with the file.
"""

import argparse
import os
import subprocess
import sys
import tempfile

GOLD = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLD))
sys.path.insert(0, os.path.dirname(GOLD))

if __name__ == "__main__":
    import test_operator_trace as T

    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="65f5409")
    ap.add_argument("--out", default=T.GOLDEN)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.parent, "vipe_amd/csrc", "include"], check=True, capture_output=True)
        subprocess.run(["tar", "-x", "-C", tmp], input=tar.stdout, check=True)
        text = T.trace(os.path.join(tmp, "vipe_amd", "csrc"), tmp, calls_switch="2")
    open(a.out, "w").write(text)
    print("wrote", a.out, len(text), "bytes,", len(T.configurations(text)), "blocks")
