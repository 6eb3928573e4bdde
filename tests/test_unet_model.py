"""tests/unet_model.py -- the float64 model that tests/test_gpu_unet_passes.py holds the device's UNet passes to -- is itself checked: against
the oracle's sixteen passes (the reference's own float32 convolutions, tests/oracle_lib.py: ref_unet_passes, checked against the reference
renderer in tests/test_unet_oracle.py), pass by pass on the ORACLE's input tensors, at frame sizes that are ragged, smaller than a tile and a
single pixel.  The model reads the weight blob with its own parser and sums in float64, so agreement here checks the parser, the schedule,
the upsample / concatenation / pooling geometry and the transfer functions.

Bound: the oracle sums the K = 9 cin + 1 terms of an accumulator in float32, in its own order; whatever the order, the result is within
K 2^-24 S of the exact sum, S = sum |a w| + |bias| (unet_model.py).  ReLU and max pooling are monotone and 1-Lipschitz and carry that
bound through (a pooled element takes the largest of its four).  The oracle evaluates the transfer functions in float32 as well: the
passes that read the images (0 and 13) get  sum |w| delta  on top, delta = t max(1, |x|) for the transferred radiance and 2^-24 |x| for
0.5 n + 0.5, and the last pass carries its bound through the inverse transfer as an envelope plus t |T(v)| (unet_model.final_image_bound).
t = 4 x the worst relative error of the float32 transfer functions with this host's libm against the float64 ones, measured over the
test's own range of arguments (unet_model.host_transfer_error; here: about 2e-7 for the forward function, 2e-6 for the inverse up to an
argument of 1, more beyond it -- the exponential stretches the argument's rounding).

Inputs: cornell_lights, 4 samples per pixel, rendered by the host build of the kernels at the frame size of the case.  Every tensor
compared has more than 5 % non-zero entries at all five sizes with this scene (at 1 x 1 the padded remainder of the 16 x 16 tensors is
ReLU(bias) and what the network makes of it), so no other scene or sample count was needed.
"""
import numpy as np
import pytest

import oracle_lib as O
import unet_model as M
import util
from ray_amd import hip

pytestmark = pytest.mark.skipif(not (O.have_ref() and O.have_hostsim()), reason="oracle/_ref or the host build is not built")

SIZES = [(64, 48), (17, 33), (16, 16), (15, 9), (1, 1)]


@pytest.fixture(scope="module")
def weights():
    return O.ref_unet_weights()


def _frame(w, h, spp=4):
    ctx = O.hostsim_context(w, h, util.golden_scene("cornell_lights"), pmj=util.pmj())
    for it in range(1, spp + 1):
        ctx.render(it)
    return ctx.readback(hip.BUF_RAW), ctx.readback(hip.BUF_BASE_COLOR), ctx.readback(hip.BUF_DEPTH_NORMALS)


@pytest.mark.parametrize("w,h", SIZES)
def test_every_pass_of_the_model_against_the_oracle(w, h, weights):
    full, base, dn = _frame(w, h)
    assert np.isfinite(full).all() and full[..., :3].min() >= 0.0
    refs = [O.ref_unet_passes(full, base, dn, p) for p in range(16)]
    model = M.UNetModel(w, h, *weights)
    t_in = M.LIBM_FACTOR * M.host_transfer_error("in", float(full[..., :3].max()))
    lines = []
    for p, d in enumerate(M.PASSES):
        for t in (d.a, d.b):
            if t >= 0:
                model.load(t, refs[t])  # the oracle's own inputs: nothing compounds
        r = model.run_pass(p, None, full, base, dn)
        bound = M.terms(p) * 2.0 ** -24 * r.S
        if d.img:
            x = np.abs(model.tensors[M.IMAGES])
            delta = np.zeros_like(x)
            delta[..., 0:3] = t_in * np.maximum(1.0, x[..., 0:3])
            delta[..., 6:9] = 2.0 ** -24 * x[..., 6:9]
            slack = model.image_slack(p, delta)
            bound = bound + slack
        if p < 15:
            ref = refs[p]
            assert ref.shape == model.tensors[d.out].shape, (p, ref.shape)
            assert not ref[0].any() and not ref[-1].any() and not ref[:, 0].any() and not ref[:, -1].any(), p
            got, want = ref[1:-1, 1:-1].astype(np.float64), r.value
        else:
            assert refs[15].shape == (h, w, 4) and np.array_equal(refs[15][..., 3], full[..., 3])
            t_out = M.LIBM_FACTOR * M.host_transfer_error("out", float(r.pre.max()))
            bound = M.final_image_bound(r.pre, bound, t_out)
            got, want = refs[15][..., :3].astype(np.float64), r.value
        assert got.shape == want.shape == bound.shape, (p, got.shape, want.shape, bound.shape)
        err = np.abs(got - want)
        ratio = float((err / np.maximum(bound, 1e-300)).max())
        lines.append(f"pass {p:2d}: K {M.terms(p):5d}  max |err| {float(err.max()):.2e}  worst err / bound {ratio:.3f}  non-zero {float((got != 0).mean()):.2f}")
        assert (err <= bound).all(), (p, ratio, np.unravel_index((err / np.maximum(bound, 1e-300)).argmax(), err.shape))
        assert (got != 0).mean() > 0.05, (p, "a dead tensor would make the comparison meaningless")  # (of what is compared: the interior)
    print(f"{w}x{h}: t_in {t_in:.2e}\n" + "\n".join(lines))


def test_the_stand_in_weights_are_halves(weights):
    """the f16 form's bound (test_gpu_unet_passes.py) takes the weights as exact in half precision: products of two halves are exact in float32"""
    w = weights[0]
    with np.errstate(over="ignore"):
        assert np.array_equal(w, w.astype(np.float16).astype(np.float32))
    for W, bias in M.parse_weights(*weights):
        assert (W != 0).mean() > 0.9 and (bias != 0).mean() > 0.9
