"""Layered passes with a pixel's layers adjacent in the per-iteration buffers (RAYHIP_LAYER_LAYOUT=1, the interleaved form of rt_base.h's
Layering, folded by k_accumulate_interleaved) against whole layers side by side (RAYHIP_LAYER_LAYOUT=0, k_accumulate) and against the same
iterations rendered one by one.  The layout moves where a ray's radiance and aux values wait for the accumulate step, nothing else: every
image must be the same bits -- BUF_RAW, BUF_VARIANCE, BUF_BASE_COLOR, BUF_DEPTH_NORMALS and BUF_FINAL.

Shapes: a frame whose width is no multiple of 8 or of the accumulate strip (100 x 52; a pass of 70 layers has 64 layer columns and two
rows), and a wide flat one (4100 x 6) whose 16-bit limit gives 65535 / 4100 = 15 columns, 8 after rounding to whole 128-byte lines, so that
passes of 7 / 9 layers sit just below / above one virtual row, 14 / 16 fill two, and 64 / 70 take eight / nine; 70 layers are also two
accumulate launches (MAX_BATCH = 64) that split a virtual row between them."""
import numpy as np
import pytest

import util
from ray_amd import hip

pytestmark = pytest.mark.gpu

SCENES = ["cornell_principled", "cornell_instances"]
BUFS = (hip.BUF_RAW, hip.BUF_VARIANCE, hip.BUF_BASE_COLOR, hip.BUF_DEPTH_NORMALS, hip.BUF_FINAL)
SMALL, WIDE = (100, 52), (4100, 6)
WIDE_COLS = 65535 // WIDE[0] // 8 * 8  # layer columns of the wide frame's passes (make_layering, rt_base.h)
COUNTS = {SMALL: (2, 64, 70), WIDE: (2, WIDE_COLS - 1, WIDE_COLS + 1, 14, 16, 64, 70)}
RECT = (8, 16, 40, 24)  # off the 8x8 tile grid of the ray generator and off the accumulate strips


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


def images(ctx):
    return [ctx.readback(buf) for buf in BUFS]


def assert_same(got, ref, what):
    for buf, a, b in zip(BUFS, got, ref):
        assert np.array_equal(a, b), (what, buf, int((a != b).any(axis=-1).sum()), "pixels differ")


def context(gpu_lib, monkeypatch, name, size, layout=None, samples=None, split=None):
    for var, val in (("RAYHIP_LAYER_LAYOUT", layout), ("RAYHIP_RAYGEN_SAMPLES", samples), ("RAYHIP_SHADE_SPLIT", split)):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, str(val))
    ctx = util.make_context(gpu_lib, name, *size)
    for var in ("RAYHIP_LAYER_LAYOUT", "RAYHIP_RAYGEN_SAMPLES", "RAYHIP_SHADE_SPLIT"):
        monkeypatch.delenv(var, raising=False)
    return ctx


_one_by_one = {}


def one_by_one(gpu_lib, name, size):
    """iterations 1 .. 70 of the full frame rendered singly, the images after each count the tests ask for (computed once, never changed)"""
    key = (name, size)
    if key not in _one_by_one:
        ctx = util.make_context(gpu_lib, name, *size)
        snaps = {}
        for it in range(1, max(COUNTS[size]) + 1):
            ctx.render(it)
            if it in COUNTS[size]:
                snaps[it] = images(ctx)
        _one_by_one[key] = snaps
    return _one_by_one[key]


@pytest.mark.parametrize("size", [SMALL, WIDE], ids=["100x52", "4100x6"])
@pytest.mark.parametrize("name", SCENES)
def test_pass_sizes_around_a_virtual_row(gpu_lib, monkeypatch, name, size):
    """render_batch(1, n) for n = 2, one less / one more than the layer columns of the frame, 64, and 70 (two accumulate launches): the
    interleaved layout, the side-by-side layout and the single iterations agree"""
    ref = one_by_one(gpu_lib, name, size)
    for n in COUNTS[size]:
        for layout in (1, 0):
            ctx = context(gpu_lib, monkeypatch, name, size, layout=layout)
            assert ctx.max_batch() == min(512, (65535 // size[0]) * (65535 // size[1]))
            ctx.render_batch(1, n)
            assert_same(images(ctx), ref[n], (name, size, n, "layout", layout))


# Two schedules, each from a fresh context.  (A full-frame batch that FOLLOWS passes over a rect is not compared: the pixels outside the
# rect are then behind the iteration count -- required_samples < iteration -- which single iterations wake up one iteration later, while
# a batch decides liveness once in the ray generator; the side-by-side layout differs from single iterations there as well, measured
# before this test was written.  rayhip_render_batch documents the same limit for adaptive sampling.)
FULL = ((1, 16), (17, 6), (23, 64))  # 6: no multiple of S = 4 / 16 / 64, the plain order of the ray generator
RECTS = ((1, 12), (13, 16))           # both over RECT


def schedule(ctx, passes, rect, shard):
    if shard:
        ctx.set_shard(32, 2, 1)
    for first, n in passes:
        ctx.render_batch(first, n, rect=rect)


_schedule_ref = {}


def schedule_ref(gpu_lib, name, passes, rect, shard):
    key = (name, passes, rect, shard)
    if key not in _schedule_ref:
        ctx = util.make_context(gpu_lib, name, *SMALL)
        if shard:
            ctx.set_shard(32, 2, 1)
        for it in range(1, passes[-1][0] + passes[-1][1]):
            ctx.render(it, rect=rect)
        _schedule_ref[key] = images(ctx)
    return _schedule_ref[key]


@pytest.mark.parametrize("shard", [False, True], ids=["whole", "shard_32_2_1"])
@pytest.mark.parametrize("samples", [1, 4, 16, 64])
@pytest.mark.parametrize("name", SCENES)
def test_samples_per_wavefront_rect_and_shard(gpu_lib, monkeypatch, name, samples, shard):
    """S = 1 / 4 / 16 / 64 samples of a pixel per primary wavefront: full-frame passes of 16, 6 (no multiple of S) and 64 layers, and passes
    of 12 and 16 layers over a rect off the tile grid -- on the whole frame and on rank 1 of 2 of a frame sharded in 32-pixel tiles (the
    strips of the accumulate kernel straddle tiles of both ranks: the other rank's pixels stay as they are)"""
    for passes, rect in ((FULL, None), (RECTS, RECT)):
        ref = schedule_ref(gpu_lib, name, passes, rect, shard)
        for layout in (1, 0):
            ctx = context(gpu_lib, monkeypatch, name, SMALL, layout=layout, samples=samples)
            schedule(ctx, passes, rect, shard)
            assert_same(images(ctx), ref, (name, "S", samples, "layout", layout, "shard", shard, "rect", rect))


@pytest.mark.parametrize("name", SCENES)
def test_default_context_matches(gpu_lib, monkeypatch, name):
    """no switch set: whatever layout and S a context picks by default"""
    for passes, rect in ((FULL, None), (RECTS, RECT)):
        ctx = context(gpu_lib, monkeypatch, name, SMALL)
        schedule(ctx, passes, rect, False)
        assert_same(images(ctx), schedule_ref(gpu_lib, name, passes, rect, False), (name, "default", rect))


@pytest.mark.parametrize("name", SCENES)
def test_adaptive_sampling_then_a_batch(gpu_lib, monkeypatch, name):
    """a camera with a variance threshold (its iterations go one layer at a time and park the pixels that converged), then a batch of the
    plain camera over the parked pixels: the `required < iteration` gate of the fold and of the ray generator"""
    out = []
    for layout, batched in ((1, True), (0, True), (1, False)):
        ctx = context(gpu_lib, monkeypatch, name, SMALL, layout=layout)
        cam = hip.Camera.from_buffer_copy(ctx.cam)
        cam.pass_settings.min_samples = 2
        cam.pass_settings.variance_threshold = 0.05
        if batched:
            ctx.render_batch(1, 10, cam=cam)
            ctx.render_batch(11, 16)
            ctx.render_batch(27, 8, cam=cam)
        else:
            for it in range(1, 35):
                ctx.render(it, cam=cam if (it <= 10 or it >= 27) else None)
        out.append(images(ctx))
    req_parked = (out[2][1] < 0.05).all(axis=-1)  # (variance below the threshold in every channel: the pixel was parked)
    assert req_parked.any() and not req_parked.all(), "the scene must park some pixels and keep some"
    assert_same(out[0], out[2], (name, "interleaved vs one by one"))
    assert_same(out[1], out[2], (name, "side by side vs one by one"))


@pytest.mark.parametrize("split", [13, 29])
def test_both_primary_shade_kernels_write_their_layer(gpu_lib, monkeypatch, split):
    """the shade stage's launch forms pinned (RAYHIP_SHADE_SPLIT): 13, the split form whose k_surface writes the primary pixel, and 29, the
    fused k_surface_scatter -- the layered write of each lands where the fold looks for it"""
    name = "cornell_principled"
    ref = one_by_one(gpu_lib, name, WIDE)
    for layout in (1, 0):
        ctx = context(gpu_lib, monkeypatch, name, WIDE, layout=layout, split=split, samples=64)
        ctx.render_batch(1, 64)
        assert_same(images(ctx), ref[64], (name, "split", split, "layout", layout))
