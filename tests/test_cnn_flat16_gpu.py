"""conv_flat16_kernel (classifier-pipeline_amd/csrc/cpx_cnn_flat.hip): stage 4's stride-1 3x3 layer in fp16x2 on flattened
bands with 16x16x32 products, and its switch CPX_CNN_FLAT16 (read when a handle is created; 0 = conv_bf3flat_kernel).

Single layers through cpx_conv2d, 256 -> 256 channels in 2 groups, N = 2, output prefilled with NaN, the four variants of
test_cnn_gpu.py::test_conv2d_matches_torch (prologue + affine + ReLU; affine + residual; all of them; bias only), each
against a float64 computation of the same variant.  Criterion (test_bf16x3_is_f32_accurate's): err = max |got - want| /
mag, mag = the magnitude the output accumulates (|activated x| * |k| through the affine, + |bias| + |residual|);
err <= 2 err_f32 + 2^-24 and err < 4e-6, err_f32 measured in the same test on the float32 kernel.  That a shape takes the new
kernel is checked by the switch: a handle created under CPX_CNN_FLAT16=0 gives other bits (K = 32 per product pairs two
16-channel chunks: another float32 summation order) and meets the same criterion.

Map shapes, H x W (flat_pays admits each: the bands fit the 256-pixel patch and the flattened tiling wastes less than the
rectangular bands):
  27 x 27  five full bands and a ragged one, fragments wrapping rows at every offset
  9 x 11   less than one band
  13 x 13  the second band is 41 positions
  13 x 29  for 5 x 29, which flat_pays does not admit (145 positions fill two bands and two 4 x 32 rectangles alike: nothing
           gained); 13 rows is the smallest height at 29 columns where the flattened tiling pays (3 bands against 4 x 128)
  17 x 30  the widest row the 256-pixel patch admits (8 staged rows x 32 pixels = 256 exactly); 17 rows is the smallest
           height at 30 columns where the flattened tiling pays (4 bands against 5 x 128)
  50 x 3   a fragment of 16 positions spans six rows
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(27, 27), (9, 11), (13, 13), (13, 29), (17, 30), (50, 3)]
TOL = 4e-6


def _engine_under(value):
    from cpx.engine import TrackEngine

    old = os.environ.get("CPX_CNN_FLAT16")
    os.environ["CPX_CNN_FLAT16"] = value
    try:
        return TrackEngine(model="lepton3")
    finally:
        if old is None:
            del os.environ["CPX_CNN_FLAT16"]
        else:
            os.environ["CPX_CNN_FLAT16"] = old


@pytest.fixture(scope="module")
def engines():
    """fresh handles created under CPX_CNN_FLAT16=1 and =0"""
    on, off = _engine_under("1"), _engine_under("0")
    yield on, off
    on.close()
    off.close()


def _conv(eng, mode, x, k, in_s=None, in_b=None, out_s=None, out_b=None, res=None, relu=False):
    """one cpx_conv2d (3x3, stride 1, SAME, 2 groups) in math mode `mode` -> float32 output"""
    import torch

    from cpx.ml_tools.wrresnet import ConvDesc, pack_conv

    dev = eng.device
    N, H, W, Cin = x.shape
    Cout = k.shape[3]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda v: None if v is None else C.c_void_p(v.data_ptr())
    keep = [up(x), up(pack_conv(k)), up(in_s), up(in_b), up(out_s), up(out_b), up(res)]
    out = torch.full((N, H, W, Cout), np.nan, dtype=torch.float32, device=dev)
    d = ConvDesc(N, H, W, Cin, Cout, 2, 3, 1, 1, 1 if relu else 0, ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                 ptr(keep[4]), ptr(keep[5]), ptr(keep[6]))
    eng.set_cnn_math(mode)
    torch.cuda.synchronize()
    assert eng.lib.cpx_conv2d(eng.h, C.byref(d)) == 0, eng._err()
    eng.synchronize()
    eng.set_cnn_math(eng.DEFAULT_CNN_MATH)
    return out.cpu().numpy()


@pytest.mark.parametrize("H,W", SHAPES)
def test_single_layer_is_f32_accurate_and_takes_the_new_kernel(engines, H, W):
    import torch
    import torch.nn.functional as F

    on, off = engines
    Cin = Cout = 256
    rng = np.random.default_rng(1000 * H + W)
    x = rng.normal(0, 1, size=(2, H, W, Cin)).astype(np.float32)
    k = rng.normal(0, 0.2, size=(3, 3, Cin // 2, Cout)).astype(np.float32)
    in_s = rng.uniform(0.5, 1.5, Cin).astype(np.float32)
    in_b = rng.normal(0, 0.3, Cin).astype(np.float32)
    out_s = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    out_b = rng.normal(0, 0.3, Cout).astype(np.float32)
    res = rng.normal(0, 1, size=(2, H, W, Cout)).astype(np.float32)
    kt = torch.from_numpy(k).double().permute(3, 2, 0, 1).contiguous()
    ch = lambda v: torch.from_numpy(v).double()[None, :, None, None]
    for variant in range(4):  # 3 = bias only
        use_pro, use_res, relu, use_scale = variant in (0, 2), variant in (1, 2), variant in (0, 2), variant != 3
        xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
        if use_pro:
            xt = F.relu(xt * ch(in_s) + ch(in_b))
        y = F.conv2d(xt, kt, None, padding=1, groups=2)
        mag = F.conv2d(xt.abs(), kt.abs(), None, padding=1, groups=2)
        if use_scale:
            y, mag = y * ch(out_s), mag * ch(out_s).abs()
        y, mag = y + ch(out_b), mag + ch(out_b).abs()
        if use_res:
            rt = torch.from_numpy(res).double().permute(0, 3, 1, 2)
            y, mag = y + rt, mag + rt.abs()
        if relu:
            y = F.relu(y)
        want, mag = y.permute(0, 2, 3, 1).numpy(), mag.permute(0, 2, 3, 1).numpy()
        args = dict(in_s=in_s if use_pro else None, in_b=in_b if use_pro else None, out_s=out_s if use_scale else None, out_b=out_b,
                    res=res if use_res else None, relu=relu)
        got = {"f32": _conv(on, "f32", x, k, **args), "flat16": _conv(on, "fp16x2", x, k, **args)}
        assert not on.cnn_last_overflow()
        got["flat32"] = _conv(off, "fp16x2", x, k, **args)
        assert not off.cnn_last_overflow()
        errs = {}
        for name, g in got.items():
            assert np.isfinite(g).all(), (name, variant)  # (the NaN prefill: every output was written)
            errs[name] = float((np.abs(g.astype(np.float64) - want) / mag).max())
        print("flat16 %2d x %2d variant %d: err / mag vs float64 %s" % (H, W, variant, errs))
        for name in ("flat16", "flat32"):
            assert errs[name] <= 2.0 * errs["f32"] + 2.0 ** -24 and errs[name] < TOL, (H, W, variant, errs)
        assert not np.array_equal(got["flat16"], got["flat32"]), (H, W, variant)  # (the switch chooses the kernel)


BLOCK_INPUTS = [(1, 160, 160), (2, 81, 81), (2, 48, 48)]  # stage 4 at 27 x 27, 14 x 14, 8 x 8


@pytest.mark.parametrize("n,h,w", BLOCK_INPUTS)
def test_blocks_route_and_switch(engines, n, h, w):
    """Every block and the head against float64 (test_cnn_blocks_gpu.py's criterion), no overflow word, on the new route and
    on the old; the stage-2 and stage-3 taps are the same bits under the switch, the stage-4 taps are not."""
    from cpx.ml_tools import wrresnet as wr
    from test_cnn_blocks_gpu import NAMES, _assert_f32_accurate, _block_errs, _input, _model, _report, _run

    x = _input(n, h, w, 300 + h)
    wt = _model(6, x)
    taps_of = {}
    for name, eng in zip(("FLAT16=1", "FLAT16=0"), engines):
        eng.set_cnn_math("fp16x2")
        net = wr.WRResNetDevice(eng, wt, 17)
        logits, taps, ovf = _run(net, eng, x)
        net.close()
        taps_of[name] = taps
        errs, herr = _block_errs(wt, x, logits, taps)
        _report("flat16 %dx%dx%d %s" % (n, h, w, name), "fp16x2", errs, herr, ovf)
        assert not ovf.any(), (name, ovf)
        assert not eng.cnn_last_overflow()
        _assert_f32_accurate((n, h, w, name), "fp16x2", errs, herr)
    for k, name in enumerate(NAMES):
        same = np.array_equal(taps_of["FLAT16=1"][k], taps_of["FLAT16=0"][k])
        assert same == (name[0] in "23"), (name, same)


def test_launch_table_under_the_switch(engines):
    from test_cnn_blocks_gpu import LAUNCH_TABLES, _launch_table

    for eng in engines:
        got = _launch_table(eng, "fp16x2")
        eng.set_cnn_math(eng.DEFAULT_CNN_MATH)
        assert got == LAUNCH_TABLES["fp16x2"], got


@pytest.mark.parametrize("where,y,xc,c", [("last ragged band", 26, 13, 5), ("halo row of band 1", 10, 20, 200)])
def test_guard_reruns_in_bf16x3(engines, where, y, xc, c):
    """27 x 27: band 5 holds positions 640..728 = rows 23..26; band 1 positions 128..255 = rows 4..9, its halo rows 3 and 10.
    One input element beyond fp16's largest finite value there: the overflow word is set and the layer's output is the
    three-plane rerun's, bit for bit the bf16x3 mode's."""
    on, _ = engines
    rng = np.random.default_rng(y)
    x = rng.normal(0, 1, size=(2, 27, 27, 256)).astype(np.float32)
    k = rng.normal(0, 0.1, size=(3, 3, 128, 256)).astype(np.float32)
    x[1, y, xc, c] = 1.0e5
    got = _conv(on, "fp16x2", x, k)
    assert on.cnn_last_overflow(), where
    want = _conv(on, "bf16x3", x, k)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want), where
