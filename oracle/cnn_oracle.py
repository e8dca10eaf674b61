"""TEST INFRASTRUCTURE ONLY -- plain PyTorch (CPU, float32) restatement of the reference's
WR-ResNet forward, the checker for the MFMA kernels.

PARITY UNPINNED against TensorFlow: neither TensorFlow nor the released model weights exist in
the build container, so what is pinned is the architecture as written in
src/ml_tools/resnet/wr_resnet.py:5-98 and src/ml_tools/kerasmodel.py:308-350: grouped (groups=2)
3x3 convolutions with bias and TensorFlow "SAME" padding (surplus at the bottom / right), strides
1 / 2 / 3, pre-activation basic blocks, 1x1 "valid" strided projection shortcuts, Keras
BatchNormalization (eps 1e-3, inference statistics), global average pooling, dense + sigmoid.
Weights use the Keras layouts of cpx.ml_tools.wrresnet (HWIO kernels).
"""

import numpy as np
import torch
import torch.nn.functional as F

BN_EPS = 1e-3
GROUPS = 2


def _conv(x, w, name, stride, same):
    k = torch.from_numpy(w[name + "/kernel"])  # [kh, kw, Cin/g, Cout]
    b = torch.from_numpy(w[name + "/bias"])
    wt = k.permute(3, 2, 0, 1).contiguous()    # [Cout, Cin/g, kh, kw]
    kh = k.shape[0]
    if same:
        H, W = x.shape[2], x.shape[3]
        Ho, Wo = -(-H // stride), -(-W // stride)
        ph = max((Ho - 1) * stride + kh - H, 0)
        pw = max((Wo - 1) * stride + kh - W, 0)
        x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    return F.conv2d(x, wt, b, stride=stride, padding=0, groups=GROUPS)


def _bn(x, w, name):
    g, b = torch.from_numpy(w[name + "/gamma"]), torch.from_numpy(w[name + "/beta"])
    m, v = torch.from_numpy(w[name + "/moving_mean"]), torch.from_numpy(w[name + "/moving_variance"])
    return (x - m[None, :, None, None]) / torch.sqrt(v[None, :, None, None] + BN_EPS) * g[None, :, None, None] + \
        b[None, :, None, None]


def forward(w, x_nhwc, return_features=False):
    """x_nhwc: float32 [N,S,S,2] -> (logits, probs) numpy [N, n_labels]."""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32)).permute(0, 3, 1, 2)
        x = _conv(x, w, "conv1_1", 1, True)
        for stage in (2, 3, 4):
            for d in range(3):
                b = "%db%d" % (stage, d)
                s = (stage - 1) if d == 0 else 1
                shortcut = x
                y = F.relu(_bn(x, w, "bn%s_branch2a" % b))
                y = _conv(y, w, "res%s_branch2a" % b, s, True)
                y = F.relu(_bn(y, w, "bn%s_branch2b" % b))
                y = _conv(y, w, "res%s_branch2b" % b, 1, True)
                if d == 0:
                    shortcut = _conv(shortcut, w, "shortcut%d" % stage, s, False)
                x = F.relu(y + shortcut)
        x = F.relu(_bn(x, w, "final_bn"))
        feat = x.mean(dim=(2, 3))
        # head variants (kerasmodel.py:337-345): Dense(relu) layers of dense_sizes, then sigmoid or softmax
        h, k = feat, 0
        while "dense_%d/kernel" % k in w:
            h = F.relu(h @ torch.from_numpy(w["dense_%d/kernel" % k]) + torch.from_numpy(w["dense_%d/bias" % k]))
            k += 1
        logits = h @ torch.from_numpy(w["prediction/kernel"]) + torch.from_numpy(w["prediction/bias"])
        probs = torch.softmax(logits, dim=1) if str(w.get("prediction/activation", "sigmoid")) == "softmax" \
            else torch.sigmoid(logits)
        if return_features:
            return logits.numpy(), probs.numpy(), feat.numpy()
        return logits.numpy(), probs.numpy()


def calibrate_bn(w, x_nhwc):
    """Set every BatchNorm's moving statistics to the batch statistics of a calibration batch (what
    training would have produced), so that seeded random weights give O(1) activations / logits."""
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32)).permute(0, 3, 1, 2)

        def fit(t, name):
            w[name + "/moving_mean"] = t.mean(dim=(0, 2, 3)).numpy().astype(np.float32)
            w[name + "/moving_variance"] = t.var(dim=(0, 2, 3), unbiased=False).numpy().astype(np.float32) + 1e-2

        x = _conv(x, w, "conv1_1", 1, True)
        for stage in (2, 3, 4):
            for d in range(3):
                b = "%db%d" % (stage, d)
                s = (stage - 1) if d == 0 else 1
                shortcut = x
                fit(x, "bn%s_branch2a" % b)
                y = F.relu(_bn(x, w, "bn%s_branch2a" % b))
                y = _conv(y, w, "res%s_branch2a" % b, s, True)
                fit(y, "bn%s_branch2b" % b)
                y = F.relu(_bn(y, w, "bn%s_branch2b" % b))
                y = _conv(y, w, "res%s_branch2b" % b, 1, True)
                if d == 0:
                    shortcut = _conv(shortcut, w, "shortcut%d" % stage, s, False)
                x = F.relu(y + shortcut)
        fit(x, "final_bn")
    return w


# ---- float64 per-block restatement (tests/test_cnn_blocks_gpu.py) -----------------------------------------------------
# Each function takes and returns NHWC float64 numpy arrays and also returns `mag`, the magnitude float32 rounding errors
# of the device's computation of the same values are relative to: every operand taken as |.| and propagated through the
# same layers, so that a float32-accurate kernel stays within a few 2^-24 of mag, element by element.

def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).permute(0, 3, 1, 2)


def _np64(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _conv64(x, w, name, stride, same, absolute=False, bias=True):
    """_conv in float64 on NCHW float64; absolute=True: conv(x, |kernel|) + |bias| (x is taken as given)."""
    k = torch.from_numpy(w[name + "/kernel"]).double()
    b = torch.from_numpy(w[name + "/bias"]).double() * (1.0 if bias else 0.0)
    if absolute:
        k, b = k.abs(), b.abs()
    wt = k.permute(3, 2, 0, 1).contiguous()
    kh = k.shape[0]
    if same:
        H, W = x.shape[2], x.shape[3]
        Ho, Wo = -(-H // stride), -(-W // stride)
        ph = max((Ho - 1) * stride + kh - H, 0)
        pw = max((Wo - 1) * stride + kh - W, 0)
        x = F.pad(x, (pw // 2, pw - pw // 2, ph // 2, ph - ph // 2))
    return F.conv2d(x, wt, b, stride=stride, padding=0, groups=GROUPS)


def _bn_affine64(w, name):
    """BatchNorm as x * scale + shift, float64, per channel [1, C, 1, 1]."""
    g, b = (torch.from_numpy(w[name + "/" + k]).double() for k in ("gamma", "beta"))
    m, v = (torch.from_numpy(w[name + "/" + k]).double() for k in ("moving_mean", "moving_variance"))
    s = g / torch.sqrt(v + BN_EPS)
    return s[None, :, None, None], (b - m * s)[None, :, None, None]


def _block64_t(w, stage, d, a, a_mag):
    b = "%db%d" % (stage, d)
    s = (stage - 1) if d == 0 else 1
    s_a, t_a = _bn_affine64(w, "bn%s_branch2a" % b)
    u = F.relu(a * s_a + t_a)
    u_mag = u.abs() + (s_a.abs() * a_mag if a_mag is not None else 0.0)
    # conv 2a without its bias; the bias and BatchNorm 2b folded into one affine, as the device takes them
    za = _conv64(u, w, "res%s_branch2a" % b, s, True, bias=False)
    Ma = _conv64(u_mag, w, "res%s_branch2a" % b, s, True, absolute=True, bias=False)
    s_b, t_b = _bn_affine64(w, "bn%s_branch2b" % b)
    sa = s_b
    ta = torch.from_numpy(w["res%s_branch2a/bias" % b]).double()[None, :, None, None] * s_b + t_b
    m = F.relu(za * sa + ta)
    y = _conv64(m, w, "res%s_branch2b" % b, 1, True)
    mag = _conv64(m.abs() + sa.abs() * Ma, w, "res%s_branch2b" % b, 1, True, absolute=True)
    a_abs = a.abs() + (a_mag if a_mag is not None else 0.0)
    if d == 0:
        sc = _conv64(a, w, "shortcut%d" % stage, s, False)
        S = _conv64(a_abs, w, "shortcut%d" % stage, s, False, absolute=True)
    else:
        sc, S = a, a_abs
    return F.relu(y + sc), mag + S


def block64(w, stage, d, a):
    """Residual block (stage, d) of forward() in float64 from its NHWC block input a -> (out, mag), NHWC float64.
    mag = conv(|m| + |sa| Ma, |Wb|) + |bb| + S, where u = relu(BN_2a(a)), Ma = conv(|u|, |Wa|), m = relu(conv_2a(u) sa + ta)
    (sa, ta: conv 2a's bias and BatchNorm 2b folded), S = |a| for the identity shortcut and conv(|a|, |Wsc|) + |bsc| for
    the projection."""
    with torch.no_grad():
        out, mag = _block64_t(w, stage, d, _t64(a), None)
        return _np64(out), _np64(mag)


def first_block64(w, x):
    """conv1_1 and block 2b0 in float64 from the NHWC input image -> (out, mag).  conv1_1's output is not a tap: its
    magnitude conv(|x|, |W1|) + |b1| enters the block's as an error scale of its input (through |BN scale| into the
    branch, as it is into the shortcut)."""
    with torch.no_grad():
        xt = _t64(x)
        c = _conv64(xt, w, "conv1_1", 1, True)
        cm = _conv64(xt.abs(), w, "conv1_1", 1, True, absolute=True)
        out, mag = _block64_t(w, 2, 0, c, cm)
        return _np64(out), _np64(mag)


def head64(w, feat_in):
    """Logits in float64 from the last block's NHWC output -> (logits, mag) [N, n_labels]:
    mag = sum_c |W_cl| mean|relu(BN(x))| + |b_l|, carried through the hidden Dense layers the same way."""
    with torch.no_grad():
        s, t = _bn_affine64(w, "final_bn")
        feat = F.relu(_t64(feat_in) * s + t).mean(dim=(2, 3))
        h, e, k = feat, feat.abs(), 0
        while "dense_%d/kernel" % k in w:
            wk = torch.from_numpy(w["dense_%d/kernel" % k]).double()
            bk = torch.from_numpy(w["dense_%d/bias" % k]).double()
            h = F.relu(h @ wk + bk)
            e = e @ wk.abs() + bk.abs()
            k += 1
        wl = torch.from_numpy(w["prediction/kernel"]).double()
        bl = torch.from_numpy(w["prediction/bias"]).double()
        return (h @ wl + bl).numpy(), (e @ wl.abs() + bl.abs()).numpy()
