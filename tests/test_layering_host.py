"""The address mapping of layered passes (Layering, ray_amd/csrc/rt_base.h) checked on the host, for both forms of the virtual frame
(side by side / interleaved: RAYHIP_LAYER_LAYOUT = 0 / 1).

tests/hostsim/layering_check.cpp is a stand-alone program over rt_base.h -- the header the device kernels and the host build share.  For one
(w, h, layer count, layout) it checks that (real x, real y, layer) -> virtual xy -> buffer index is injective, stays inside the allocated
virtual frame and below 2^31, keeps both halves of the packed xy within 16 bits, and that xy_layer / xy_real invert it exactly: exhaustively
for small passes, on the corners and a seeded sample of 10^5 pixels (all layers of each) for large ones.  It also prints max_layers_for,
which must be what tests/test_gpu_parity.py::test_maximal_batch_and_row_limit_split expects of rayhip_max_batch wherever the 31-bit index
bound does not bind."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostsim", "layering_check.cpp")

CASES = [(1920, 1080, 64), (1920, 1080, 1), (3840, 2160, 64), (65, 65, 512), (96, 64, 70), (7, 5, 3)]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("layering") / "layering_check")
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", SRC, "-o", exe], check=True)
    return exe


def run(checker, w, h, count, layout):
    r = subprocess.run([checker, str(w), str(h), str(count), str(layout), "20251019"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    out = dict(line.split(None, 1) for line in r.stdout.splitlines())
    assert "ok" in out, r.stdout
    return out


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("w,h,count", CASES)
def test_mapping_is_injective_in_bounds_and_inverted(checker, w, h, count, layout):
    out = run(checker, w, h, count, layout)
    checked = int(out["ok"])
    pairs = w * h * count
    if pairs <= 1 << 22:
        assert checked == pairs  # exhaustive
    else:
        assert checked >= 50000 * count  # corners + the sample (distinct pixels of 10^5 draws), every layer of each
    geometry = out["cols"].split()  # "cols C rows R virtual W x H" without its first word
    cols, rows = int(geometry[0]), int(geometry[2])
    assert cols * rows >= count
    if layout == 1 and count > 1:
        # a pixel's layers in as few runs as the 16-bit limit allows, in whole 128-byte lines (8 slots) where the pass still fits
        widest = min(count, 65535 // w)
        lines = widest - widest % 8
        fits = lines and -(-count // lines) <= 65535 // h and lines * -(-count // lines) * w * h < 1 << 31
        assert cols == (lines if fits else widest)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("w,h", [(1920, 1080), (65, 65), (96, 64), (7, 5), (64, 48), (16, 2000), (24, 30000), (1024, 1024)])
def test_max_layers_where_the_index_bound_does_not_bind(checker, w, h, layout):
    """rayhip_max_batch = min(512, (65535 / w) * (65535 / h)) (tests/test_gpu_parity.py), in either layout"""
    expect = min(512, (65535 // w) * (65535 // h))
    assert expect * w * h < 1 << 31  # (the frames of this list: the index bound is not what limits them)
    out = run(checker, w, h, 1, layout)
    assert int(out["max_layers"]) == expect


@pytest.mark.parametrize("layout", [0, 1])
def test_max_layers_under_the_index_bound_fits(checker, layout):
    """3840x2160: 2^31 / pixels = 258 layers bound the pass before the 16-bit limit (17 x 30) does; the largest admitted pass must still
    pass the mapping check (the check fails a virtual frame of 2^31 elements or more)"""
    out = run(checker, 3840, 2160, 1, layout)
    n = int(out["max_layers"])
    assert 1 <= n <= 258
    run(checker, 3840, 2160, n, layout)
