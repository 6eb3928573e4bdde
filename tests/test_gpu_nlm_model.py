"""The NLM filter on the device (k_nlm_prepare_h, k_nlm_prepare_v, k_nlm_filter behind rayhip_denoise_nlm) against a float64 model, on
crafted images that both the device and the host build receive byte for byte through the exchange calls (tests/denoise_cases.py).

k_nlm_filter is not the per-pixel form the host build runs: 16 x 16 tiles, a 24 x 24 rim staged in LDS, an 18 x 18 distance image per
window offset, staging clamped at the right and bottom edge, a block that strides over tiles.  What is asserted: the injection returns
every image bit for bit; over a rect list that puts tile seams, frame borders, single pixels, rows and columns under the filter, the
device stays within 4 x e_ref of the model and of the host build in the filter's own domain, all four channels (e_ref: the host
build's own distance from the model on the same bytes -- both builds run the same IEEE operations in the same order and differ in expf
alone; tests/test_nlm_model_hostsim.py shows every modelled kernel error at more than 40 x e_ref); nothing outside a rect and no input
image changes; four ragged rects give the bits of the whole frame; a frame with more tiles than the launch has blocks is periodic where
its input is; FINAL is the tonemap of RAW, to the bit on the table path; and the adaptive mark is the one the model predicts."""
import numpy as np
import pytest
import torch  # noqa: F401  (FIRST: torch brings its own HIP runtime, and it must be the one that opens the device -- tests/test_gpu_comm.py)

import denoise_cases as D
import util
from ray_amd import hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu_lib():
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path, -m gpu tests cannot run here"
    return lib


@pytest.fixture(scope="module")
def hostsim_lib():
    return D.host_library()


_results = {}


def results(gpu_lib, hostsim_lib, name):
    """per rect of D.rects(): (rect, model tm, host RAW crop, device RAW crop) of case `name`, computed once"""
    if name not in _results:
        images = D.case_images(name)
        gpu, host = D.context(gpu_lib), D.context(hostsim_lib)
        out = []
        for rect in D.rects():
            crops = []
            for ctx in (host, gpu):
                D.inject(ctx, *images, tile=12)
                ctx.denoise_nlm(1, rect=rect)
                crops.append(D.crop(ctx.readback(hip.BUF_RAW), rect).copy())
            tm, _, _ = D.nlm_model(images[0], images[3], images[1], images[2], rect)
            out.append((rect, tm, crops[0], crops[1]))
        _results[name] = out
    return _results[name]


@pytest.mark.parametrize("w,h,tile", [(65, 33, 12), (D.W, D.H, 12), (65, 33, 64), (D.W, D.H, 64)])
def test_injection_round_trip(gpu_lib, w, h, tile):
    full, base, dn, variance = D.crafted(w, h, level=8.0, seed=5)
    ctx = D.context(gpu_lib, w, h)
    D.inject(ctx, full, base, dn, variance, tile=tile)
    got = D.read_all(ctx)
    for key, want in (("raw", full), ("base", base), ("dn", dn), ("variance", variance)):
        assert np.array_equal(D.bits(got[key]), D.bits(want)), key


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_filter_against_the_model(gpu_lib, hostsim_lib, name):
    worst = 0.0
    for rect, tm, host, dev in results(gpu_lib, hostsim_lib, name):
        e_ref, d = D.distance(host, tm), D.distance(dev, tm)
        print(f"{name} rect {rect}: e_ref {e_ref:.3e}, device to model {d:.3e}")
        worst = max(worst, d / (4 * max(e_ref, D.ULP)))
        assert np.isfinite(dev).all()
        assert e_ref <= D.e_ref_bound(tm), (name, rect, e_ref)
        assert d <= 4 * max(e_ref, D.ULP), (name, rect, d, e_ref)
    print(f"{name}: at most {worst:.3f} of the bound")


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_filter_against_the_host_build(gpu_lib, hostsim_lib, name):
    for rect, tm, host, dev in results(gpu_lib, hostsim_lib, name):
        e_ref = D.distance(host, tm)
        d = float(np.abs(D.filter_domain(dev) - D.filter_domain(host)).max())
        print(f"{name} rect {rect}: e_ref {e_ref:.3e}, device to host build {d:.3e}, same bits in RAW: {float((D.bits(dev) == D.bits(host)).mean()):.4f}")
        assert d <= 4 * max(e_ref, D.ULP), (name, rect, d, e_ref)


def test_pixels_outside_the_rect_and_the_inputs_keep_their_bits(gpu_lib):
    D.check_pixels_outside_the_rect(gpu_lib)


def test_partition_invariance_and_repeatability(gpu_lib):
    images = D.case_images("level8")
    whole, parts = D.context(gpu_lib), D.context(gpu_lib)
    D.inject(whole, *images, tile=12)
    D.inject(parts, *images, tile=12)
    whole.denoise_nlm(1)
    first = {buf: whole.readback(buf).copy() for buf in (hip.BUF_RAW, hip.BUF_FINAL)}
    for rect in D.PARTITION:
        parts.denoise_nlm(1, rect=rect)
    whole.denoise_nlm(1)  # (the filter reads the running mean, not RAW: the same call again)
    for buf in (hip.BUF_RAW, hip.BUF_FINAL):
        assert np.array_equal(D.bits(parts.readback(buf)), D.bits(first[buf])), buf
        assert np.array_equal(D.bits(whole.readback(buf)), D.bits(first[buf])), buf


PERIOD = 48  # three tiles: every period of a periodic frame sees the tile grid the same way


def test_more_tiles_than_blocks(gpu_lib, hostsim_lib):
    """the launch has min(tiles, 32 x CUs) blocks: on a frame of about 1.25 x that many tiles some blocks filter two tiles, others one.
    The injected images repeat every 48 x 48 pixels, so the output does wherever the filter's 8-pixel reach stays off the border."""
    blocks = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = 33
    h, w = 16 * rows, 16 * (-(-(5 * blocks // 4) // rows))
    tiles = rows * (w // 16)
    print(f"{blocks} blocks, frame {w} x {h}: {tiles} tiles, {w * h * 16 / 1e6:.1f} MB per image")
    assert tiles > blocks
    unit = D.crafted(PERIOD, PERIOD, level=8.0, seed=21)
    images = [np.ascontiguousarray(np.tile(a, (-(-h // PERIOD), -(-w // PERIOD), 1))[:h, :w]) for a in unit]
    gpu = D.context(gpu_lib, w, h)
    D.inject(gpu, *images, tile=h)
    gpu.denoise_nlm(1)
    raw, final = gpu.readback(hip.BUF_RAW), gpu.readback(hip.BUF_FINAL)
    # one interior period against the model and the host build, on a 3 x 3 period crop: the filter reaches 8 pixels, so they see the same bytes
    rect = (PERIOD, PERIOD, PERIOD, PERIOD)
    small = [np.ascontiguousarray(a[:3 * PERIOD, :3 * PERIOD]) for a in images]
    host = D.context(hostsim_lib, 3 * PERIOD, 3 * PERIOD)
    D.inject(host, *small)
    host.denoise_nlm(1, rect=rect)
    tm, _, _ = D.nlm_model(small[0], small[3], small[1], small[2], rect)
    e_ref, d = D.distance(D.crop(host.readback(hip.BUF_RAW), rect), tm), D.distance(D.crop(raw, rect), tm)
    print(f"interior period: e_ref {e_ref:.3e}, device to model {d:.3e}")
    assert e_ref <= D.e_ref_bound(tm) and d <= 4 * max(e_ref, D.ULP)
    # every period at least 48 pixels from the border has the bits of that one
    ny, nx = (h - PERIOD) // PERIOD, (w - PERIOD) // PERIOD
    assert ny >= 3 and nx >= 3
    for img in (raw, final):
        p = D.bits(img)[PERIOD:ny * PERIOD, PERIOD:nx * PERIOD].reshape(ny - 1, PERIOD, nx - 1, PERIOD, 4)
        differ = (p != p[:1, :, :1]).any(axis=(1, 3, 4))
        assert not differ.any(), f"{int(differ.sum())} of {differ.size} periods differ, the first at {tuple(np.argwhere(differ)[0])}"


def _final_check(gpu, host, raw, kw, what):
    """the device's FINAL against the host build's tonemap of the very RAW the device holds"""
    cam = D.camera(gpu.cam, **kw)
    dev_final = gpu.readback(hip.BUF_FINAL)
    zero = np.zeros_like(raw)
    D.inject(host, raw, zero, zero, zero, cam=cam)
    host_final = host.readback(hip.BUF_FINAL)
    if cam.view_transform != 0 and cam.gamma == 1.0:  # the table path: no libm call
        same = D.bits(dev_final) == D.bits(host_final)
        assert same.all(), f"{what} {kw}: {int((~same).sum())} values differ, the first at {tuple(np.argwhere(~same)[0])}"
        return
    lut, dims = D.lut_of_blob(util.golden_scene("cornell_filmic"))
    model = D.tonemap_model(raw, cam, lut, dims)
    d_host, d_dev = float(np.abs(host_final - model).max()), float(np.abs(dev_final - model).max())
    print(f"{what} {kw}: host FINAL to the float64 tonemap {d_host:.3e}, device FINAL {d_dev:.3e}")
    assert d_dev <= 4 * d_host, (what, kw, d_dev, d_host)


@pytest.mark.parametrize("kw", D.TONEMAPS, ids=D.TONEMAP_IDS)
def test_final_is_the_tonemap_of_the_filtered_raw(gpu_lib, hostsim_lib, kw):
    gpu, host = D.context(gpu_lib), D.context(hostsim_lib)
    cam = D.camera(gpu.cam, **kw)
    for name, rect in (("level8", None), ("level60", (5, 3, 33, 17))):
        D.inject(gpu, *D.case_images(name), tile=12, cam=cam)
        gpu.denoise_nlm(1, rect=rect, cam=cam)
        _final_check(gpu, host, gpu.readback(hip.BUF_RAW).copy(), kw, f"{name} {rect}")


@pytest.mark.parametrize("kw", D.TONEMAPS, ids=D.TONEMAP_IDS)
def test_tonemap_of_a_crafted_ramp(gpu_lib, hostsim_lib, kw):
    """rayhip_finish_import / k_retonemap on 0, denormals, the knee of the Standard curve, the table's cell boundaries and its last cell"""
    _, dims = D.lut_of_blob(util.golden_scene("cornell_filmic"))
    ramp = D.ramp_image(dims)
    h, w = ramp.shape[:2]
    gpu, host = D.context(gpu_lib, w, h), D.context(hostsim_lib, w, h)
    zero = np.zeros_like(ramp)
    D.inject(gpu, ramp, zero, zero, zero, cam=D.camera(gpu.cam, **kw))
    assert np.array_equal(D.bits(gpu.readback(hip.BUF_RAW)), D.bits(ramp))
    _final_check(gpu, host, ramp, kw, "ramp")


def test_the_adaptive_mark_the_filter_leaves(gpu_lib, hostsim_lib):
    """nlm_finish_pixel re-arms required_samples where the filtered variance reaches the threshold: seen through the pixels the next
    iteration samples, on the device, on the host build and as the model predicts (pixels within 4 ulp of the threshold left out)"""
    images = D.crafted(D.W, D.H, **D.ADAPTIVE_CASE)
    on_gpu = D.adaptive_changed(gpu_lib, images, D.ADAPTIVE_THRESHOLD)
    on_host = D.adaptive_changed(hostsim_lib, images, D.ADAPTIVE_THRESHOLD)
    armed, near = D.armed_prediction(images)
    print(f"armed {int(armed.sum())} of {armed.size} pixels, {int(near.sum())} within 4 ulp of the threshold; device {int(on_gpu.sum())}, host build {int(on_host.sum())}")
    assert 0.1 < armed.mean() < 0.9 and near.mean() <= 0.005
    assert np.array_equal(on_gpu[~near], on_host[~near])
    assert np.array_equal(on_gpu[~near], armed[~near])
