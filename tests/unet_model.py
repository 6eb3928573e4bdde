"""A float64 model of the UNet denoiser, pass by pass, for the tests of ray_amd/csrc/unet_kernels.hip.

Written from the description of the network in ray_amd/csrc/unet.h and rayhip_denoise.hip.h (the schedule table UNET_PASSES, the tensor
sizes, the weight blob's layout), not from any implementation: sixteen 3 x 3 convolutions with bias and ReLU over NHWC tensors that carry
a one-pixel zero border at round_up16 size, 2 x 2 max pooling on the way down, nearest-neighbour upsampling and concatenation on the way
up, an HDR transfer function on the radiance input and its inverse on the output.  No GPU, no project code: numpy, and torch's float64
conv2d on the CPU for the sums.

Besides every value the model returns the absolute-value sum  S = sum |a w| + |bias|  of the accumulator behind it: a summation of K terms
in a binary format of unit round-off u, in ANY order, is within K u S of the exact sum (to first order), which is what the tests' bounds
are made of.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

# the sixteen passes, as UNET_PASSES in rayhip_denoise.hip.h: first input (tensor id or -1), its channels, whether it is read through the
# upsample, second input, its channels, whether the three images are an input (nine channels, behind the others), output channels,
# output tensor (-1: the image), resolution divider of the pass, pooling
Pass = namedtuple("Pass", "a a_ch up b b_ch img cout out div pool")
PASSES = [
    Pass(-1, 0, 0, -1, 0, 1, 32, 0, 1, 0),
    Pass(0, 32, 0, -1, 0, 0, 32, 1, 1, 1),
    Pass(1, 32, 0, -1, 0, 0, 48, 2, 2, 1),
    Pass(2, 48, 0, -1, 0, 0, 64, 3, 4, 1),
    Pass(3, 64, 0, -1, 0, 0, 80, 4, 8, 1),
    Pass(4, 80, 0, -1, 0, 0, 96, 5, 16, 0),
    Pass(5, 96, 0, -1, 0, 0, 96, 6, 16, 0),
    Pass(6, 96, 1, 3, 64, 0, 112, 7, 8, 0),
    Pass(7, 112, 0, -1, 0, 0, 112, 8, 8, 0),
    Pass(8, 112, 1, 2, 48, 0, 96, 9, 4, 0),
    Pass(9, 96, 0, -1, 0, 0, 96, 10, 4, 0),
    Pass(10, 96, 1, 1, 32, 0, 64, 11, 2, 0),
    Pass(11, 64, 0, -1, 0, 0, 64, 12, 2, 0),
    Pass(12, 64, 1, -1, 0, 1, 64, 13, 1, 0),
    Pass(13, 64, 0, -1, 0, 0, 32, 14, 1, 0),
    Pass(14, 32, 0, -1, 0, 0, 3, -1, 1, 0),
]
TENSOR_DIV = [1, 2, 4, 8, 16, 16, 16, 8, 8, 4, 4, 2, 2, 1, 1]
TENSOR_CH = [32, 32, 48, 64, 80, 96, 96, 112, 112, 96, 96, 64, 64, 64, 32]
IMAGES = 15  # id of the 16-channel image-inputs tensor (nine channels used), as rayhip_unet_read_tensor numbers it
IMAGE_CH = 16
H_MAX = 65504.0  # largest finite half


def round_up(v, a):
    return a * ((v + a - 1) // a)


def in_channels(p):
    """(channels of the first input, of the second) as the weight blob counts them: the nine image channels are one input"""
    d = PASSES[p]
    c1 = d.a_ch if d.a >= 0 else 0
    c2 = d.b_ch if d.b >= 0 else (9 if d.img else 0)
    return c1, c2


def terms(p):
    """K: the number of terms of one accumulator of pass p (nine taps of every input channel, and the bias)"""
    return 9 * sum(in_channels(p)) + 1


def parse_weights(weights, offsets, alignment=8):
    """[(W[cout, cin_total, 3, 3], bias[cout])] of the sixteen passes, float64, from the blob that rayhip_unet_init takes: per output channel
    three rows (ky) of round_up(3 cin, alignment) floats holding [kx][c]; a pass with two inputs keeps, per output channel, the three rows
    of its first input and then the three of its second.  offsets[2 p] is where pass p's weights start, offsets[2 p + 1] its biases."""
    weights = np.asarray(weights)
    out = []
    for p, d in enumerate(PASSES):
        w_off, b_off = int(offsets[2 * p]), int(offsets[2 * p + 1])
        widths = [c for c in in_channels(p) if c]
        row = [round_up(3 * c, alignment) for c in widths]
        per_out = 3 * sum(row)
        block = weights[w_off:w_off + d.cout * per_out].astype(np.float64).reshape(d.cout, per_out)
        parts, at = [], 0
        for c, r in zip(widths, row):
            rows = block[:, at:at + 3 * r].reshape(d.cout, 3, r)[:, :, :3 * c]  # [n][ky][kx * c + channel]
            parts.append(rows.reshape(d.cout, 3, 3, c).transpose(0, 3, 1, 2))   # -> [n][channel][ky][kx]
            at += 3 * r
        out.append((np.ascontiguousarray(np.concatenate(parts, axis=1)), weights[b_off:b_off + d.cout].astype(np.float64)))
    return out


# ---- the HDR transfer function and its inverse.  The constants are the float32 values of the decimal literals the kernels are written
# with, so that this IS the real function the float32 code approximates (thresholds included).
def _f(x):
    return float(np.float32(x))


_A, _B, _C, _D, _E, _FF, _G = _f(1.41283765e+03), _f(1.64593172e+00), _f(4.31384981e-01), _f(-2.94139609e-03), _f(1.92653254e-01), \
    _f(6.26026094e-03), _f(9.98620152e-01)
_Y0, _Y1, _X0, _X1 = _f(1.57945760e-06), _f(3.22087631e-02), _f(2.23151711e-03), _f(3.70974749e-01)
_IN_SCALE, _OUT_SCALE = _f(0.318967164), _f(3.13511896)


def transfer_in_hdr(x):
    """radiance -> network input: linear near zero, a power law, then a logarithm; scaled so that the range ends near one"""
    x = np.asarray(x, dtype=np.float64)
    pos = np.maximum(x, 0.0)
    return np.where(x <= _Y0, _A * x, np.where(x <= _Y1, _B * np.power(pos, _C) + _D, _E * np.log(pos + _FF) + _G)) * _IN_SCALE


def transfer_out_hdr(v):
    """network output -> radiance: the inverse of transfer_in_hdr"""
    v = np.asarray(v, dtype=np.float64) * _OUT_SCALE
    mid = np.power(np.maximum((v - _D) / _B, 0.0), 1.0 / _C)
    with np.errstate(over="ignore"):
        return np.where(v <= _X0, v / _A, np.where(v <= _X1, mid, np.exp((v - _G) / _E) - _FF))


def image_inputs(full, base, dn):
    """[h, w, 16] float64: radiance through the transfer function, base colour, depth-normals as 0.5 n + 0.5, seven zeros"""
    h, w = full.shape[:2]
    out = np.zeros((h, w, IMAGE_CH))
    out[..., 0:3] = transfer_in_hdr(full[..., :3])
    out[..., 3:6] = np.asarray(base, dtype=np.float64)[..., :3]
    out[..., 6:9] = 0.5 * np.asarray(dn, dtype=np.float64)[..., :3] + 0.5
    return out


# what run_pass hands back: `value` is what the pass wrote ([rows, columns, channels] of `rect`, which is (x, y, w, h) in the OUTPUT's
# resolution -- the interior coordinates of the output tensor, or of the image for pass 15), `S` the absolute-value sum behind every
# element (for a pooled element the largest of its four), `pre` the ReLU'd accumulator (equal to `value` except for pass 15, where
# `value` is transfer_out_hdr(pre))
PassResult = namedtuple("PassResult", "value S pre rect")


class UNetModel:
    def __init__(self, w, h, weights, offsets, alignment=8):
        self.w, self.h = w, h
        self.wr, self.hr = round_up(w, 16), round_up(h, 16)
        self.params = parse_weights(weights, offsets, alignment)
        self.tensors = [np.zeros((self.hr // TENSOR_DIV[t] + 2, self.wr // TENSOR_DIV[t] + 2, TENSOR_CH[t])) for t in range(15)]
        self.tensors.append(np.zeros((self.hr + 2, self.wr + 2, IMAGE_CH)))
        self.image = np.zeros((h, w, 3))  # RGB of the filtered image (pass 15)

    def load(self, t, array):
        """tensor t (15: the image inputs) <- a [rows, columns, channels] array with its border, e.g. what the device holds"""
        assert array.shape == self.tensors[t].shape, (t, array.shape, self.tensors[t].shape)
        self.tensors[t] = np.array(array, dtype=np.float64)

    def pass_rect(self, p, rect):
        """(x, y, w, h) of `rect` (frame pixels) in pass p's own resolution"""
        x, y, w, h = rect
        if p < 15:
            w, h = round_up(w, 16), round_up(h, 16)
        div = PASSES[p].div
        return x // div, y // div, (w + div - 1) // div, (h + div - 1) // div

    def out_rect(self, p, rect):
        """... in the resolution of what the pass writes"""
        x, y, w, h = self.pass_rect(p, rect)
        return (x // 2, y // 2, w // 2, h // 2) if PASSES[p].pool else (x, y, w, h)

    def _patch(self, t, rx, ry, rw, rh, up, channels):
        """pixels rx - 1 .. rx + rw, ry - 1 .. ry + rh of tensor t at the pass's resolution, borders included; `up`: the tensor has half that
        resolution, pixel X of the pass is the tensor's pixel floor(X / 2) (-1 and the far border fall on the tensor's own border)"""
        xs, ys = np.arange(rx - 1, rx + rw + 1), np.arange(ry - 1, ry + rh + 1)
        if up:
            xs, ys = xs // 2, ys // 2
        return self.tensors[t][np.ix_(ys + 1, xs + 1)][..., :channels]

    def run_pass(self, p, rect=None, full=None, base=None, dn=None):
        """pass p on `rect` (frame pixels; default: the frame) over the current tensors.  A pass that takes the images computes the image
        tensor from full / base / dn first when they are given, and otherwise uses the one that is loaded."""
        d = PASSES[p]
        rect = (0, 0, self.w, self.h) if rect is None else tuple(rect)
        if d.img and full is not None:
            self.tensors[IMAGES][:] = 0.0
            self.tensors[IMAGES][1:self.h + 1, 1:self.w + 1] = image_inputs(full, base, dn)
        rx, ry, rw, rh = self.pass_rect(p, rect)
        parts = []
        if d.a >= 0:
            parts.append(self._patch(d.a, rx, ry, rw, rh, d.up, d.a_ch))
        if d.b >= 0:
            parts.append(self._patch(d.b, rx, ry, rw, rh, 0, d.b_ch))
        if d.img:
            parts.append(self._patch(IMAGES, rx, ry, rw, rh, 0, 9))
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts, axis=-1).transpose(2, 0, 1)))[None]  # [1, cin, rh + 2, rw + 2]
        W, bias = self.params[p]
        assert x.shape[1] == W.shape[1]
        Wt, bt = torch.from_numpy(W), torch.from_numpy(bias)
        acc = F.conv2d(x, Wt, bt)[0].numpy().transpose(1, 2, 0)                      # [rh, rw, cout]
        S = F.conv2d(x.abs(), Wt.abs(), bt.abs())[0].numpy().transpose(1, 2, 0)
        pre = np.maximum(acc, 0.0)
        if d.pool:
            pre = pre.reshape(rh // 2, 2, rw // 2, 2, d.cout).max(axis=(1, 3))
            S = S.reshape(rh // 2, 2, rw // 2, 2, d.cout).max(axis=(1, 3))
        ox, oy, ow, oh = self.out_rect(p, rect)
        assert pre.shape == (oh, ow, d.cout)
        if d.out >= 0:
            value = pre
            self.tensors[d.out][oy + 1:oy + oh + 1, ox + 1:ox + ow + 1] = value
        else:
            value = transfer_out_hdr(pre)
            self.image[oy:oy + oh, ox:ox + ow] = value
        return PassResult(np.ascontiguousarray(value), np.ascontiguousarray(S), np.ascontiguousarray(pre), (ox, oy, ow, oh))

    def image_slack(self, p, delta, rect=None):
        """what a perturbation of the image tensor by at most `delta` ([rows, columns, 16], border included) can move the accumulators of pass
        p (one that takes the images) by: sum |w| delta over the nine image channels, per element of the output as in PassResult"""
        d = PASSES[p]
        assert d.img
        rect = (0, 0, self.w, self.h) if rect is None else tuple(rect)
        rx, ry, rw, rh = self.pass_rect(p, rect)
        xs, ys = np.arange(rx, rx + rw + 2), np.arange(ry, ry + rh + 2)
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(delta, dtype=np.float64)[np.ix_(ys, xs)][..., :9].transpose(2, 0, 1)))[None]
        W = torch.from_numpy(np.ascontiguousarray(np.abs(self.params[p][0][:, -9:])))
        return np.ascontiguousarray(F.conv2d(x, W)[0].numpy().transpose(1, 2, 0))


# ---- what the tests' bounds are made of -----------------------------------------------------------------------------------------------
def _libm():
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    for name in ("powf", "logf", "expf"):
        getattr(m, name).restype = ctypes.c_float
        getattr(m, name).argtypes = [ctypes.c_float] * (2 if name == "powf" else 1)
    return m


def transfer_in_hdr_f32(x, m=None):
    """transfer_in_hdr as the float32 code evaluates it -- every operation rounded to float32, powf / logf from the host's libm"""
    m = m or _libm()
    f = np.float32
    out = np.empty(len(x), dtype=np.float32)
    for i, v in enumerate(np.asarray(x, dtype=np.float32)):
        if v <= f(_Y0):
            r = f(_A) * v * f(_IN_SCALE)
        elif v <= f(_Y1):
            r = (f(_B) * f(m.powf(v, f(_C))) + f(_D)) * f(_IN_SCALE)
        else:
            r = (f(_E) * f(m.logf(v + f(_FF))) + f(_G)) * f(_IN_SCALE)
        out[i] = r
    return out


def transfer_out_hdr_f32(v, m=None):
    m = m or _libm()
    f = np.float32
    out = np.empty(len(v), dtype=np.float32)
    for i, x in enumerate(np.asarray(v, dtype=np.float32)):
        x = x * f(_OUT_SCALE)
        if x <= f(_X0):
            r = x / f(_A)
        elif x <= f(_X1):
            r = f(m.powf((x - f(_D)) / f(_B), f(1.0) / f(_C)))
        else:
            r = f(m.expf((x - f(_G)) / f(_E))) - f(_FF)
        out[i] = r
    return out


_measured = {}


def host_transfer_error(which, hi):
    """worst relative error |float32 evaluation - float64| / |float64| of transfer_in_hdr ("in") or transfer_out_hdr ("out") with the host's
    libm, over 12000 float32 arguments spread logarithmically over (1e-9, hi] (`hi` is rounded up to a multiple of 1/4, so that the
    figure does not move with the last digit of a test's range)"""
    hi = float(np.ceil(max(hi, 0.25) * 4.0) / 4.0)
    if (which, hi) not in _measured:
        x = np.unique(np.concatenate([[0.0], np.geomspace(1e-9, hi, 12000)]).astype(np.float32))
        got, exact = (transfer_in_hdr_f32(x), transfer_in_hdr(x)) if which == "in" else (transfer_out_hdr_f32(x), transfer_out_hdr(x))
        ok = exact != 0.0
        assert np.array_equal(got[~ok], exact[~ok]) and np.isfinite(got).all(), (which, hi)
        _measured[(which, hi)] = float((np.abs(got[ok].astype(np.float64) - exact[ok]) / np.abs(exact[ok])).max())
    return _measured[(which, hi)]


LIBM_FACTOR = 4.0  # the device's libm may be a few ulp looser than the host's: t = LIBM_FACTOR x the host's measured worst relative error


def final_image_bound(pre, b, t):
    """a bound b on the accumulator carried through the inverse transfer function T as an envelope, plus the evaluation error of T itself:
    max(|T(v + b) - T(v)|, |T(v - b) - T(v)|) + t |T(v)|"""
    T = transfer_out_hdr(pre)
    return np.maximum(np.abs(transfer_out_hdr(pre + b) - T), np.abs(transfer_out_hdr(pre - b) - T)) + t * np.abs(T)
