"""The host side of scene deformation (ray_amd/csrc/rayhip_deform.hip.h) makes the same calls in the same order and refuses in the same
words as before its copies were consolidated: tools/deform_trace.py walks every entry point of the file on its accepting path and through
every distinct refusal, with RAYHIP_TRACE_UPLOAD set, and prints the phase stamps (one per synchronising step of a call; the millisecond
figures masked), the return codes and the error texts.  tests/golden/deform_trace.txt is that text as the library wrote it BEFORE the
consolidation -- recorded twice from the parent commit, the two runs equal -- so it is compared line for line, and is not to be
re-recorded from a library whose host side changed since: a difference is a changed return code, text, stamp or order of steps."""
import os
import subprocess
import sys

import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import util
from ray_amd import api, hip

pytestmark = [pytest.mark.gpu]

TOOL = os.path.join(util.ROOT, "tools", "deform_trace.py")
RECORDED = os.path.join(util.GOLDEN, "deform_trace.txt")


def test_the_calls_and_the_words_are_the_recorded_ones():
    assert hip.Library().device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    if not os.path.exists(api.HIP_HOST_LIB):
        pytest.skip("libray_hip.so not built (needs the reference tree at build time)")  # (cornell_lights is built through it)
    run = subprocess.run([sys.executable, TOOL], capture_output=True, text=True, timeout=300)  # (a fresh process: one trace, one C stderr)
    assert run.returncode == 0, run.stderr[-4000:]
    got = run.stdout.splitlines()
    with open(RECORDED) as f:
        want = f.read().splitlines()
    first = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
    marker = next((line for line in reversed(want[:first + 1]) if line.startswith("== ")), "")
    assert got == want, (f"line {first + 1}, under '{marker}': recorded {want[first:first + 1]}, now {got[first:first + 1]}; "
                         f"{len(want)} lines recorded, {len(got)} now")
