"""Helper (not a test): the NumPy restatement of the fp16x2 convolution's arithmetic as include/cpx.h fixes it
(CPX_GRAPH_RANGE / CPX_GRAPH_CONV_F16X2): the per-sample power-of-two range, the per-channel filter scaling, the two
splits (astype(np.float16): round to nearest even) and the three plane products, summed in float64.  It reads nothing of
cpx/ml_tools/tflite_graph.py: the planner's packing is held against it, not the other way round."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = np.float32


FAMILIES = ("uniform", "wide", "relu", "spike", "tiny")


def families(rng, shape):
    """The five input families of the arithmetic tests, name -> float64 [N, H, W, C] (cast to float32 by the caller): uniform
    +-1; +-1 times 2^U(-20, 0); ReLU-like values up to 1e4; +-1 with one channel at 3e38; +-1e-30."""
    sign = rng.choice(np.array([-1.0, 1.0]), size=shape)
    spike = sign.copy()
    spike[..., min(5, shape[-1] - 1)] = 3e38
    return {
        "uniform": rng.uniform(-1, 1, size=shape),
        "wide": sign * 2.0 ** rng.uniform(-20, 0, size=shape),
        "relu": np.maximum(rng.normal(0, 3000, size=shape), 0).clip(0, 1e4),
        "spike": spike,
        "tiny": sign * 1e-30,
    }


def range_params(x):
    """One sample's view (any shape, float32) -> (up, down) as float32."""
    x = np.asarray(x, F32)
    m = F32(np.fmax.reduce(np.abs(x).reshape(-1))) if x.size else F32(0)
    if not (m > 0) or not np.isfinite(m):
        return F32(1), F32(1)
    e = int(np.frexp(m)[1])   # m = f * 2^e, f in [0.5, 1)
    k = min(15 - e, 100)   # (e <= 128: k >= -113, no lower clamp)
    return F32(np.ldexp(F32(1), k)), F32(np.ldexp(F32(1), -k))


def split(v):
    """float32 -> (hi, lo) fp16 planes: hi = RNE(v), lo = RNE(v - hi), the difference exact in float32."""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(F32)).astype(np.float16)
    return hi, lo


def filter_exponents(w_ohwi):
    """kw[c] = clamp(4 - e, -100, 100), max |w[c]| = f * 2^e with f in [0.5, 1): max |w[c]| * 2^kw[c] in [8, 16); an
    all-zero (or non-finite) filter: 0."""
    w = np.asarray(w_ohwi, F32)
    m = np.abs(w.reshape(w.shape[0], -1)).max(axis=1)
    kw = np.zeros(w.shape[0], np.int32)
    for c, v in enumerate(m):
        if v > 0 and np.isfinite(v):
            kw[c] = min(max(4 - int(np.frexp(v)[1]), -100), 100)
    return kw


def split_filter(w_ohwi):
    """-> (wh, wl, kw): the fp16 planes of w * 2^kw[c] and the exponents."""
    w = np.asarray(w_ohwi, F32)
    kw = filter_exponents(w)
    with np.errstate(over="ignore", invalid="ignore"):
        ws = (w * np.ldexp(F32(1), kw).astype(F32)[:, None, None, None]).astype(F32)
    wh, wl = split(ws)
    return wh, wl, kw


def stage(x_nhwc):
    """[N, H, W, C] float32 -> (xh, xl, up[N], down[N]): every sample scaled by its own `up` and split."""
    x = np.asarray(x_nhwc, F32)
    prm = [range_params(s) for s in x]
    up = np.array([p[0] for p in prm], F32)
    down = np.array([p[1] for p in prm], F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        xs = (x * up[:, None, None, None]).astype(F32)
    xh, xl = split(xs)
    return xh, xl, up, down


def activate(v, act):
    """CPX_GRAPH_ACT_* in float32: 0 none, 1 RELU, 3 RELU6, 16 swish, 17 logistic."""
    v = np.asarray(v, F32)
    if act == 1:
        return np.maximum(v, F32(0))
    if act == 3:
        return np.minimum(np.maximum(v, F32(0)), F32(6))
    if act in (16, 17):
        with np.errstate(over="ignore"):
            s = (F32(1) / (F32(1) + np.exp(-v, dtype=F32))).astype(F32)
        return (v * s).astype(F32) if act == 16 else s
    assert act == 0, act
    return v


def _conv64(x, w, strides, pads):
    pt, pl, pb, pr = pads
    xin = F.pad(torch.as_tensor(np.asarray(x, np.float64)).permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xin, torch.as_tensor(np.asarray(w, np.float64)).permute(0, 3, 1, 2), None, stride=strides)
    return y.permute(0, 2, 3, 1).numpy()


def conv(x_nhwc, w_ohwi, strides=(1, 1), pads=(0, 0, 0, 0), scale=None, shift=None, act=0, parts=False):
    """CONV_F16X2 of a dense input.  pads: top, left, bottom, right.  -> float32 [N, Ho, Wo, Cout]; parts=True: also a dict
    with the float64 accumulator `acc` (of the scaled planes), the staged planes and the largest staged |xh|.
    acc = sum (wl xh + wh xl + wh xh) in float64, rounded to float32 once (the device accumulates in float32 in its own
    order: equal where every partial sum is exact); out = act(float32(acc * float32(down * 2^-kw)) * scale + shift)."""
    xh, xl, up, down = stage(x_nhwc)
    wh, wl, kw = split_filter(w_ohwi)
    acc = _conv64(xh, wl, strides, pads) + _conv64(xl, wh, strides, pads) + _conv64(xh, wh, strides, pads)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        acc32 = acc.astype(F32)
        f = (down[:, None, None, None] * np.ldexp(F32(1), -kw).astype(F32)[None, None, None, :]).astype(F32)
        v = (acc32 * f).astype(F32)
        if scale is not None:
            v = (v * np.asarray(scale, F32)).astype(F32)
        if shift is not None:
            v = (v + np.asarray(shift, F32)).astype(F32)
    out = activate(v, act)
    if parts:
        return out, {"acc": acc, "xh": xh, "xl": xl, "wh": wh, "wl": wl, "kw": kw, "up": up, "down": down,
                     "max_xh": float(np.abs(xh.astype(np.float64)).max()) if xh.size else 0.0}
    return out


def conv_float64(x_nhwc, w_ohwi, strides=(1, 1), pads=(0, 0, 0, 0)):
    """-> (the float64 convolution, sum |x| |w|): the yardstick and the scale of a rounding error."""
    x, w = np.asarray(x_nhwc, np.float64), np.asarray(w_ohwi, np.float64)
    return _conv64(x, w, strides, pads), _conv64(np.abs(x), np.abs(w), strides, pads)
