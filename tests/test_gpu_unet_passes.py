"""Every launch of the UNet denoiser (ray_amd/csrc/unet_kernels.hip behind rayhip_denoise_unet) on its own, against the float64 model of
tests/unet_model.py (checked against the reference in tests/test_unet_model.py), on small frames and on regions.

Pass by pass, each on the DEVICE's own inputs: before pass p runs, the tensors it reads are read back and loaded into the model; the model
runs pass p in float64; what the device wrote is compared with that.  (The image-inputs tensor, id 15, is written by the very call that
consumes it: it is read back after the call, checked against the float64 transfer function, and handed to the model.)  Nothing compounds,
so the bound of one launch can be derived instead of guessed.  With K = 9 cin + 1 terms per accumulator and S = sum |a w| + |bias|:

  f32 form   |got - model| <= K 2^-23 S.  Any order of summation in float32 is within K 2^-24 S; 2^-23 allows the matrix unit's adders to
             truncate instead of rounding to nearest.  That factor is reasoned, not measured.
  f16 form   tensors and weights are halves, their products exact in float32, the accumulators float32 as above; the result is rounded to
             a half and saturates at 65504:  |got - min(model, 65504)| <= K 2^-23 S + 2^-11 |model|.
  ReLU and 2 x 2 max pooling are monotone and 1-Lipschitz: the bound goes through them, a pooled element takes the largest of its four.
  pass 15    (both forms: float32 RGB through the inverse transfer function T)  with b = K 2^-23 S:
             max(|T(v + b) - T(v)|, |T(v - b) - T(v)|) + t |T(v)|.
  tensor 15  the transferred radiance, base colour and 0.5 n + 0.5 within t max(1, |x|) of the float64 values; the f16 form adds 2^-11 |x|.
  t          the device libm's relative error in powf / logf / expf is not documented to the ulp, so: LIBM_FACTOR = 4 times the worst
             relative error of the same float32 formulas with the host's libm against float64, measured over the range of arguments of
             the case (unet_model.host_transfer_error).  Measured on glibc 2.35: forward function 1.8e-7 .. 2.2e-7 up to radiance 4096
             (t = 7e-7 .. 9e-7); inverse 2.7e-6 up to an argument of 2, 4.2e-6 up to 4 (t = 1.1e-5, 1.7e-5: the exponential stretches the
             rounding of its argument).  The factor 4 allows for a device libm a few ulp looser than glibc.
  borders    the one-pixel border of every tensor stays zero; everything outside the pass's (rounded) rect is, bit for bit, what it was
             before the launch -- for a freshly sized tensor: zero.

Every test prints, per pass, the worst ratio of error to bound it saw.

The frames: cornell_lights at 4 samples per pixel, with the radiance overwritten (set_raw_device) by a pattern whose last row and last column
are distinct and large (about 1e3): a kernel that drops or duplicates an edge texel cannot pass.
"""
import numpy as np
import pytest

import oracle_lib as O
import unet_model as M
import util
from ray_amd import hip

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -23
U16 = 2.0 ** -11

_weights = None


def _ref_weights():
    global _weights
    if _weights is None:
        if not O.have_ref():
            pytest.fail("oracle/_ref/libray_ref.so is missing on the GPU box")
        _weights = O.ref_unet_weights()
    return _weights


def _ctx(w, h):
    lib = hip.Library()
    assert lib.device_count() > 0, "no HIP device: the product has no CPU path"
    ctx = util.make_context(lib, "cornell_lights", w, h)
    ctx.unet_init(*_ref_weights(), 8)
    return ctx


def _frame(ctx, spp=4):
    """render, then overwrite the radiance: (full, base, dn) as the device holds them"""
    import torch
    w, h = ctx.w, ctx.h
    ctx.render_batch(1, spp)
    full = ctx.readback(hip.BUF_RAW).copy()
    rgb = np.arange(3, dtype=np.float32)
    full[h - 1, :, :3] = 1000.0 + 7.0 * np.arange(w, dtype=np.float32)[:, None] + rgb          # last row: 1000, 1007, ...
    full[:, w - 1, :3] = 1700.0 + 11.0 * np.arange(h, dtype=np.float32)[:, None] + rgb         # last column (and the corner): 1700, 1711, ...
    dev = torch.from_numpy(full).cuda()
    ctx.set_raw_device(dev.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(ctx.readback(hip.BUF_RAW), full)
    return full, ctx.readback(hip.BUF_BASE_COLOR), ctx.readback(hip.BUF_DEPTH_NORMALS)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _border_is_zero(t):
    return not (_bits(t[0]).any() or _bits(t[-1]).any() or _bits(t[:, 0]).any() or _bits(t[:, -1]).any())


def _check_image_tensor(img, frame, half):
    """tensor 15 against the float64 transfer function; returns the worst error / bound"""
    full, base, dn = frame
    h, w = full.shape[:2]
    want = M.image_inputs(full, base, dn)
    t_in = M.LIBM_FACTOR * M.host_transfer_error("in", float(full[..., :3].max()))
    bound = t_in * np.maximum(1.0, np.abs(want)) + (U16 * np.abs(want) if half else 0.0)
    got = img[1:h + 1, 1:w + 1].astype(np.float64)
    err = np.abs(got - want)
    assert (err <= bound).all(), ("image inputs", float((err / bound).max()), np.unravel_index((err / bound).argmax(), err.shape))
    if not half:
        assert np.array_equal(got[..., 3:6], want[..., 3:6])  # base colour is copied
    outside = img.copy()
    outside[1:h + 1, 1:w + 1, :9] = 0.0
    assert not _bits(outside).any(), "the image tensor is zero outside the image and in its seven spare channels"
    return float((err / bound).max())


class Runner:
    """one context and one model side by side"""

    def __init__(self, ctx, frame, half):
        self.ctx, self.frame, self.half = ctx, frame, half
        self.model = M.UNetModel(ctx.w, ctx.h, *_ref_weights())
        self.worst = [0.0] * 16
        self.worst_img = 0.0
        ctx.unet_precision(half)

    def run_pass(self, p, rect=None, fresh=False):
        """`fresh`: the tensors of this frame size do not exist yet -- what the pass leaves outside its rect must be zero"""
        ctx, model, d = self.ctx, self.model, M.PASSES[p]
        for t in (d.a, d.b):
            if t >= 0:
                model.load(t, ctx.unet_read_tensor(t))
        if d.out < 0:
            before = ctx.readback(hip.BUF_RAW)
        elif fresh:
            before = np.zeros(model.tensors[d.out].shape, dtype=np.float32)
        else:
            before = ctx.unet_read_tensor(d.out)
        ctx.denoise_unet(p, rect)
        if d.img:
            img = ctx.unet_read_tensor(M.IMAGES)
            self.worst_img = max(self.worst_img, _check_image_tensor(img, self.frame, self.half))
            model.load(M.IMAGES, img)
        r = model.run_pass(p, rect)
        ox, oy, ow, oh = r.rect
        b = M.terms(p) * U32 * r.S
        if d.out >= 0:
            after = ctx.unet_read_tensor(d.out)
            assert after.shape == before.shape, (p, after.shape, before.shape)
            assert _border_is_zero(after), (p, "border")
            got = after[oy + 1:oy + oh + 1, ox + 1:ox + ow + 1].astype(np.float64)
            want = np.minimum(r.value, M.H_MAX) if self.half else r.value
            bound = b + (U16 * np.abs(r.value) if self.half else 0.0)
            untouched = np.ones(after.shape[:2], dtype=bool)
            untouched[oy + 1:oy + oh + 1, ox + 1:ox + ow + 1] = False
            assert np.array_equal(_bits(after)[untouched], _bits(before)[untouched]), (p, rect, "wrote outside its rect")
        else:
            after = ctx.readback(hip.BUF_RAW)
            got = after[oy:oy + oh, ox:ox + ow, :3].astype(np.float64)
            want = r.value
            t_out = M.LIBM_FACTOR * M.host_transfer_error("out", float(r.pre.max()))
            bound = M.final_image_bound(r.pre, b, t_out)
            keep = before.copy()
            keep[oy:oy + oh, ox:ox + ow, :3] = after[oy:oy + oh, ox:ox + ow, :3]
            assert np.array_equal(_bits(after), _bits(keep)), (rect, "the last pass wrote alpha, or outside its rect")
        assert got.shape == want.shape == bound.shape, (p, got.shape, want.shape, bound.shape)
        assert np.isfinite(got).all(), p
        err = np.abs(got - want)
        ratio = err / np.maximum(bound, 1e-300)
        self.worst[p] = max(self.worst[p], float(ratio.max()))
        if not (err <= bound).all():
            y, x, n = (int(v) for v in np.unravel_index(ratio.argmax(), ratio.shape))
            pytest.fail(f"pass {p} rect {rect} {'f16' if self.half else 'f32'} form: error / bound {float(ratio.max()):.3g} at row {oy + y} column {ox + x} "
                        f"channel {n} of the output (row {y} column {x} of the rect): got {got[y, x, n]!r}, model {want[y, x, n]!r}, "
                        f"bound {bound[y, x, n]:.3g}; {int((err > bound).sum())} of {err.size} elements out of bound")
        return r

    def run_all(self, rect=None, fresh=False):
        for p in range(16):
            self.run_pass(p, rect, fresh=fresh and p == 0)
            if fresh and p == 0:  # the tensors were sized by that call: all but the one it wrote are zero, borders included
                for t in range(1, 15):
                    assert not _bits(self.ctx.unet_read_tensor(t)).any(), (t, "a freshly sized tensor is zero")

    def report(self, title):
        print(f"{title} ({'f16' if self.half else 'f32'} form): worst error / bound  image inputs {self.worst_img:.3f}  passes "
              + " ".join(f"{v:.3f}" for v in self.worst))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("w,h", [(16, 16), (17, 33), (15, 9), (1, 1), (64, 48)])
def test_every_pass_on_the_full_frame(w, h, half):
    """16 x 16: the 1/16-resolution tensors are 1 x 1.  17 x 33: ragged by one in both axes, and an upsample whose source is the border.
    15 x 9 and 1 x 1: smaller than a tile.  64 x 48: more than one workgroup in every pass down to 1/4 resolution."""
    ctx = _ctx(w, h)
    run = Runner(ctx, _frame(ctx), half)
    run.run_all(fresh=True)
    run.report(f"{w}x{h}")


RECTS = [(16, 16, 40, 30), (48, 32, 32, 32), (0, 0, 80, 64), (64, 48, 16, 16)]


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_regions_region_major_then_pass_major(half):
    """DenoiseImage(pass, region) as a tiled renderer drives it: all sixteen passes of one rect, then the next rect, over tensors the
    previous rects left dirty (their writes spill to the rounded-up size and the neighbours read across the seams); then the same rects
    pass-major.  The model is handed the device's tensors before every launch, so whatever is dirty is dirty on both sides."""
    ctx = _ctx(80, 64)
    run = Runner(ctx, _frame(ctx), half)
    with pytest.raises(RuntimeError, match="corner is a multiple of 16"):
        ctx.denoise_unet(0, (8, 16, 40, 30))
    first = True
    for rect in RECTS:
        for p in range(16):
            run.run_pass(p, rect, fresh=first)
            first = False
    run.report("80x64, region-major")
    run.worst = [0.0] * 16
    for p in range(16):
        for rect in RECTS:
            run.run_pass(p, rect)
    run.report("80x64, pass-major")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_resize_gives_zeroed_tensors_of_the_new_size(half):
    ctx = _ctx(80, 64)
    for i, (w, h) in enumerate([(80, 64), (17, 33), (80, 64)]):
        if i:
            ctx.resize(w, h)
        run = Runner(ctx, _frame(ctx), half)
        run.run_all(fresh=True)
        run.report(f"resize to {w}x{h}")


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_all_passes_in_one_call_equal_sixteen_calls(half):
    """pass = -1 runs the same launches in the same order (the f16 form writes the image tensor once instead of twice): bit for bit"""
    ctx = _ctx(64, 48)
    frame = _frame(ctx)
    ctx.unet_precision(half)

    def state():
        return [_bits(ctx.unet_read_tensor(t)) for t in range(16)] + [_bits(ctx.readback(hip.BUF_RAW)), _bits(ctx.readback(hip.BUF_FINAL))]

    for p in range(16):
        ctx.denoise_unet(p)
    single = state()
    ctx.resize(32, 32)  # (new, zeroed tensors for the second run: equality below is its own doing)
    ctx.resize(64, 48)
    again = _frame(ctx)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(frame, again))
    ctx.denoise_unet(-1)
    at_once = state()
    for t, (a, b) in enumerate(zip(single, at_once)):
        assert np.array_equal(a, b), (t, int((a != b).sum()))
    assert single[14].any() and single[16].any()
