"""The NLM filter's float64 model (tests/denoise_cases.py) against the host build of rt_denoise.h, on crafted images injected byte for byte.

What is asserted here, without a GPU: the injection harness returns every image bit for bit; the host build stays within a few float32
roundings of the model in the filter's own domain (this distance, e_ref, is what tests/test_gpu_nlm_model.py takes the device's bounds
from); every mutant of the model -- one typical kernel error each -- is seen by some case and rect at ten times the device's bound; a
frame filtered as four ragged rects has the bits of the frame filtered whole; pixels outside a rect keep theirs; and the adaptive mark
the filter leaves is the one the model's filtered variance predicts."""
import numpy as np
import pytest

import denoise_cases as D
import util
from ray_amd import hip


@pytest.fixture(scope="module")
def lib():
    return D.host_library()


_results = {}


def host_results(lib, name):
    """per rect of D.rects(): (model tm, host RAW crop, e_ref) of case `name`, computed once"""
    if name not in _results:
        images = D.case_images(name)
        ctx = D.context(lib)
        out = []
        for rect in D.rects():
            D.inject(ctx, *images, tile=12)
            ctx.denoise_nlm(1, rect=rect)
            raw = D.crop(ctx.readback(hip.BUF_RAW), rect).copy()
            tm, _, _ = D.nlm_model(images[0], images[3], images[1], images[2], rect)
            out.append((tm, raw, D.distance(raw, tm)))
        _results[name] = out
    return _results[name]


@pytest.mark.parametrize("w,h,tile", [(65, 33, 12), (64, 64, 64), (17, 5, 128), (D.W, D.H, 12)])
def test_injection_round_trip(lib, w, h, tile):
    full, base, dn, variance = D.crafted(w, h, level=8.0, seed=5)
    ctx = D.context(lib, w, h)
    D.inject(ctx, full, base, dn, variance, tile=tile)
    got = D.read_all(ctx)
    for key, want in (("raw", full), ("base", base), ("dn", dn), ("variance", variance)):
        assert np.array_equal(D.bits(got[key]), D.bits(want)), key
    # and the three-image meaning of mask 0 is what it was: the variance image stays out of it
    assert ctx.owned_bytes(0, 2, 0) * 4 == ctx.owned_bytes(D.MASK, 2, 0) * 3


def test_the_library_is_the_plain_host_build_plus_its_variance_image(lib):
    """tests/hostsim_nlm compiles tests/hostsim/hostsim.cpp as it is: a rendered and filtered frame has the bits libhostsim.so gives, mask 0
    packs the same three images, and mask 15 exports what pack() lays out"""
    import oracle_lib as O
    assert O.have_hostsim(), "tests/hostsim is not built (run __graft_entry__.build())"
    plain = hip.Library(O.HOSTSIM_LIB, prefix="hostsim_")
    frames, packed = [], []
    for library in (plain, lib):
        ctx = D.context(library, D.W, D.H, "cornell_basic")
        util.render_frames(ctx, 3)
        ctx.denoise_nlm(3, rect=(5, 3, 33, 17))
        frames.append([ctx.readback(b).copy() for b in (hip.BUF_RAW, hip.BUF_FINAL, hip.BUF_BASE_COLOR, hip.BUF_DEPTH_NORMALS)])
        ctx.set_shard(12, 2, 1)
        buf = np.zeros(ctx.owned_bytes(0, 2, 1) // 4, dtype=np.float32)
        ctx.export_owned(0, buf.ctypes.data, buf.nbytes)
        packed.append(buf)
    assert all(np.array_equal(D.bits(a), D.bits(b)) for a, b in zip(*frames)) and np.array_equal(D.bits(packed[0]), D.bits(packed[1]))
    images = D.case_images("level8")
    ctx = D.context(lib)
    D.inject(ctx, *images, tile=12)
    for rank in (0, 1):
        ctx.set_shard(12, 2, rank)
        buf = np.full(ctx.owned_bytes(D.MASK, 2, rank) // 4, -1.0, dtype=np.float32)
        ctx.export_owned(D.MASK, buf.ctypes.data, buf.nbytes)
        assert np.array_equal(D.bits(buf), D.bits(D.pack(list(images[:3]) + [images[3]], D.W, D.H, 12, 2, rank))), rank
        only = np.full(ctx.owned_bytes(hip.REDUCE_VARIANCE, 2, rank) // 4, -1.0, dtype=np.float32)
        ctx.export_owned(hip.REDUCE_VARIANCE, only.ctypes.data, only.nbytes)
        assert np.array_equal(D.bits(only), D.bits(D.pack([images[3]], D.W, D.H, 12, 2, rank))), rank
    with pytest.raises(RuntimeError):
        ctx.export_owned(D.MASK, buf.ctypes.data, 16)


@pytest.mark.parametrize("name", sorted(D.CASES))
def test_host_build_against_the_model(lib, name):
    for rect, (tm, raw, e_ref) in zip(D.rects(), host_results(lib, name)):
        print(f"{name} rect {rect}: e_ref {e_ref:.3e} (max |tm| {float(np.abs(tm).max()):.3f})")
        assert e_ref <= D.e_ref_bound(tm), (name, rect, e_ref)


def test_the_f32_twin_is_the_same_function(lib):
    """the restatement run in float32 is another float32 evaluation of the same operations: as close to the float64 one as the host build"""
    images = D.case_images("level8")
    for rect in (D.rects()[0], D.rects()[8]):
        tm64, raw64, var64 = D.nlm_model(images[0], images[3], images[1], images[2], rect)
        tm32, raw32, var32 = D.nlm_model(images[0], images[3], images[1], images[2], rect, dtype=np.float32)
        assert tm32.dtype == np.float32 and raw32.dtype == np.float32 and var32.dtype == np.float32
        assert float(np.abs(tm32 - tm64).max()) <= D.e_ref_bound(tm64)


@pytest.mark.parametrize("mutant", D.MUTANTS)
def test_every_mutant_is_seen(lib, mutant):
    """some case and rect of the list shows the mutant at more than 10 x the device's bound (4 e_ref) at a compared pixel"""
    best, where = 0.0, None
    for name in sorted(D.CASES):
        images = D.case_images(name)
        for rect, (tm, _, e_ref) in zip(D.rects(), host_results(lib, name)):
            _, raw_m, _ = D.nlm_model(images[0], images[3], images[1], images[2], rect, mutant=mutant)
            margin = D.distance(raw_m, tm) / (4 * max(e_ref, D.ULP))
            if margin > best:
                best, where = margin, (name, rect)
        if best > 10.0:
            break
    print(f"{mutant}: {best:.1f} x the device's bound at {where}")
    assert best > 10.0, (mutant, best)


def test_partition_invariance(lib):
    images = D.case_images("level8")
    whole, parts = D.context(lib), D.context(lib)
    D.inject(whole, *images, tile=12)
    D.inject(parts, *images, tile=12)
    whole.denoise_nlm(1)
    for rect in D.PARTITION:
        parts.denoise_nlm(1, rect=rect)
    for buf in (hip.BUF_RAW, hip.BUF_FINAL):
        assert np.array_equal(D.bits(whole.readback(buf)), D.bits(parts.readback(buf))), buf


def test_pixels_outside_the_rect_keep_their_bits(lib):
    D.check_pixels_outside_the_rect(lib)


def test_final_is_the_tonemap_of_raw(lib):
    """FINAL inside the rect is tonemap(RAW): a second context handed that RAW as its running mean computes the same bits"""
    images = D.case_images("level8")
    ctx, twin = D.context(lib), D.context(lib)
    for cam in (D.camera(ctx.cam, gamma=1.0), D.camera(ctx.cam, view_transform=0, gamma=2.2)):
        D.inject(ctx, *images, tile=12, cam=cam)
        ctx.denoise_nlm(1, cam=cam)
        raw = ctx.readback(hip.BUF_RAW).copy()
        D.inject(twin, raw, images[1], images[2], images[3], tile=64, cam=cam)
        assert np.array_equal(D.bits(twin.readback(hip.BUF_FINAL)), D.bits(ctx.readback(hip.BUF_FINAL)))


@pytest.mark.parametrize("kw", D.TONEMAPS, ids=D.TONEMAP_IDS)
def test_tonemap_model_on_the_ramp(lib, kw):
    """the host build's tonemap of the crafted ramp against tonemap_model: float32 roundings apart (the distance the device's bound on
    FINAL is taken from)"""
    lut, dims = D.lut_of_blob(util.golden_scene("cornell_filmic"))
    ramp = D.ramp_image(dims)
    h, w = ramp.shape[:2]
    ctx = D.context(lib, w, h)
    cam = D.camera(ctx.cam, **kw)
    zero = np.zeros_like(ramp)
    D.inject(ctx, ramp, zero, zero, zero, tile=64, cam=cam)
    final = ctx.readback(hip.BUF_FINAL)
    model = D.tonemap_model(ramp, cam, lut, dims)
    d = float(np.abs(final.astype(np.float64) - model).max())
    print(f"{kw}: host FINAL within {d:.3e} of the float64 tonemap on {w} x {h} ramp pixels, dims {dims}")
    assert d <= D.tonemap_bound(cam, lut, dims)
    assert np.array_equal(D.bits(ctx.readback(hip.BUF_RAW)), D.bits(ramp))


def test_the_adaptive_mark_is_the_one_the_model_predicts(lib):
    images = D.crafted(D.W, D.H, **D.ADAPTIVE_CASE)
    changed = D.adaptive_changed(lib, images, D.ADAPTIVE_THRESHOLD)
    armed, near = D.armed_prediction(images)
    print(f"armed {int(armed.sum())} of {armed.size} pixels, {int(near.sum())} within 4 ulp of the threshold")
    assert 0.1 < armed.mean() < 0.9, "the threshold does not cut the frame"
    assert near.mean() <= 0.005
    assert np.array_equal(changed[~near], armed[~near])
