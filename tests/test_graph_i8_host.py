"""The full-integer arithmetic of the graph executor (classifier-pipeline_amd/csrc/cpx_graph_i8_core.h: SRDHM, RDivPOT,
MBQM, the float32 -> int8 quantise, DEQUANTIZE, the ADD chain, MUL, MEAN's finish, the rounding division) compiled for the
HOST and held, bit for bit, to the NumPy restatement (tests/tflite_eval_i8.py, written from the arithmetic's text).  The
planner's QuantizeMultiplier against hand values.  Needs no GPU; the product never loads this build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tflite_eval_i8 as te8

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "graph_i8_host.cpp")
INCLUDES = ["-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc"), "-I", os.path.join(REPO, "include")]
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = tmp_path_factory.mktemp("graph_i8") / "libgraph_i8_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-ffp-contract=off", *INCLUDES, SRC, "-o", str(out)])
    return C.CDLL(str(out))


def i32(a):
    return np.ascontiguousarray(a, np.int32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def call(fn, *arrays, scalars=(), out_dtype=np.int32):
    n = arrays[0].size
    out = np.zeros(n, out_dtype)
    fn(*[ptr(a) for a in arrays], *scalars, C.c_int(n), ptr(out))
    return out


def test_srdhm(host):
    rng = np.random.default_rng(1)
    edge = np.array([I32_MIN, I32_MIN + 1, -3, -1, 0, 1, 3, 2 ** 30, -2 ** 30, I32_MAX - 1, I32_MAX], np.int64)
    a = np.concatenate([np.repeat(edge, edge.size), rng.integers(I32_MIN, I32_MAX + 1, 100000)])
    b = np.concatenate([np.tile(edge, edge.size), rng.integers(I32_MIN, I32_MAX + 1, 100000)])
    got = call(host.srdhm_host, i32(a), i32(b))
    assert np.array_equal(got, te8.srdhm(a, b))
    # INT32_MIN * INT32_MIN saturates; ties of both signs with M = 2^30 (x / 2), by hand from the nudges: a positive tie
    # goes up ((2^30 + 2^30) / 2^31 = 1), a negative one towards zero ((-2^30 + 1 - 2^30) / 2^31 truncates to 0)
    assert call(host.srdhm_host, i32([I32_MIN]), i32([I32_MIN]))[0] == I32_MAX
    assert list(call(host.srdhm_host, i32([1, -1, 3, -3, 0]), i32([2 ** 30] * 5))) == [1, 0, 2, -1, 0]


def test_rdivpot(host):
    rng = np.random.default_rng(2)
    xs = np.array([I32_MIN, -(2 ** 31 - 1), -5, -3, -2, -1, 0, 1, 2, 3, 5, I32_MAX], np.int64)
    x = np.concatenate([np.repeat(xs, 32), rng.integers(I32_MIN, I32_MAX + 1, 100000)])
    e = np.concatenate([np.tile(np.arange(32), xs.size), rng.integers(0, 32, 100000)])
    got = call(host.rdivpot_host, i32(x), i32(e))
    assert np.array_equal(got, te8.rdivpot(x, e))
    assert list(call(host.rdivpot_host, i32([1, -1, 3, -3, 5, -5]), i32([1] * 6))) == [1, -1, 2, -2, 3, -3]
    # every exponent from 1 to 31 on a tie of either sign: +-2^(e - 1) -> +-1
    es = np.arange(1, 32)
    assert np.array_equal(call(host.rdivpot_host, i32(2 ** (es - 1)), i32(es)), np.ones(31, np.int32))
    assert np.array_equal(call(host.rdivpot_host, i32(-(2 ** (es - 1))), i32(es)), -np.ones(31, np.int32))


def test_mbqm(host):
    rng = np.random.default_rng(3)
    n = 100000
    shift = rng.integers(-31, 31, n)
    left = np.maximum(shift, 0)
    x = (rng.integers(I32_MIN, I32_MAX + 1, n) >> left).astype(np.int64)   # x * 2^left stays in int32
    m = rng.integers(2 ** 30, 2 ** 31, n)
    # the edges: zero, +-(2^31 - 1) at no left shift, the ties of M = 2^30 (a multiplier of exactly 1/2 and 1/4)
    xe = np.array([0, I32_MAX, -I32_MAX, 1, -1, 3, -3, 5, -5, 1, -1, 3, -3], np.int64)
    me = np.array([2 ** 30 + 12345, I32_MAX, I32_MAX] + [2 ** 30] * 10, np.int64)
    se = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, -1, -1, -1, -1], np.int64)
    x, m, shift = np.concatenate([xe, x]), np.concatenate([me, m]), np.concatenate([se, shift])
    got = call(host.mbqm_host, i32(x), i32(m), i32(shift))
    assert np.array_equal(got, te8.mbqm(x, m, shift))
    # by hand: x / 2 as SRDHM's ties above; x / 4 rounds twice (1 -> SRDHM 1 -> RDivPOT(1, 1) = 1; -3 -> -1 -> -1)
    assert list(got[3:13]) == [1, 0, 2, -1, 3, -2, 1, 0, 1, -1]


def test_quantize_and_dequantize(host):
    rng = np.random.default_rng(4)
    host.quantize_f32_host.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int, C.c_void_p]
    host.dequantize_i8_host.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int, C.c_void_p]
    for s, z in ((np.float32(0.05), -7), (np.float32(1.0), 0), (np.float32(0.0123), 127), (np.float32(3.0), -128)):
        ties = (np.arange(-300, 300) + 0.5).astype(np.float32) * s
        x = np.concatenate([ties, rng.normal(0, 40 * s, 100000).astype(np.float32),
                            np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 0.49999997 * s], np.float32)])
        got = np.zeros(x.size, np.int32)
        host.quantize_f32_host(ptr(x), C.c_float(s), z, x.size, ptr(got))
        want = te8.quantize_f32(x, s, z)
        assert np.array_equal(got, want) and got.min() >= -128 and got.max() <= 127
        assert got[ties.size + 100000] == z   # NaN
        q = np.arange(-128, 128, dtype=np.int32)
        back = np.zeros(256, np.float32)
        host.dequantize_i8_host(ptr(q), C.c_float(s), z, 256, ptr(back))
        assert np.array_equal(back, te8.dequantize(q, s, z))


def _header(**kw):
    from cpx.ml_tools.tflite_graph_i8 import header, unpack_header

    return np.ascontiguousarray(unpack_header(header(**kw)))


def test_add_mul_mean_chains(host):
    from cpx.ml_tools.tflite_graph_i8 import quantize_multiplier

    rng = np.random.default_rng(5)
    q1, q2 = np.meshgrid(np.arange(-128, 128), np.arange(-128, 128))
    q1, q2 = i32(q1.reshape(-1)), i32(q2.reshape(-1))
    for p1, p2, po, act in (((np.float32(0.02), -5), (np.float32(0.74), 11), (np.float32(0.5), -20), 0),
                            ((np.float32(1.3), 127), (np.float32(0.035), -128), (np.float32(0.9), 3), 1),
                            ((np.float32(0.01), 0), (np.float32(0.01), 0), (np.float32(0.011), -128), 3)):
        lo, hi = te8.clamp_bounds(act, *po)
        twice = 2.0 * max(float(p1[0]), float(p2[0]))
        (m1, e1), (m2, e2) = quantize_multiplier(float(p1[0]) / twice), quantize_multiplier(float(p2[0]) / twice)
        mo, eo = quantize_multiplier(twice / (2.0 ** 20 * float(po[0])))
        h = _header(z_in=p1[1], z_in1=p2[1], z_out=po[1], lo=lo, hi=hi, m0=m1, s0=e1, m1=m2, s1=e2, mo=mo, so=eo, left=20)
        for sign in (1, -1):
            got = np.zeros(q1.size, np.int32)
            host.add_i8_host(ptr(q1), ptr(q2), sign, ptr(h), q1.size, ptr(got))
            assert np.array_equal(got, te8.add_i8(q1, q2, sign, p1, p2, po, lo, hi))
        m, e = quantize_multiplier(float(p1[0]) * float(p2[0]) / float(po[0]))
        h = _header(z_in=p1[1], z_in1=p2[1], z_out=po[1], lo=lo, hi=hi, m0=m, s0=e)
        got = np.zeros(q1.size, np.int32)
        host.mul_i8_host(ptr(q1), ptr(q2), ptr(h), q1.size, ptr(got))
        assert np.array_equal(got, te8.mul_i8(q1, q2, p1, p2, po, lo, hi))
    acc = i32(np.concatenate([np.arange(-50, 51), rng.integers(-10 ** 6, 10 ** 6, 1000)]))
    cnt = i32(np.concatenate([np.tile([1, 2, 3, 4, 6, 9, 49], 15)[:101], rng.integers(1, 500, 1000)]))
    assert np.array_equal(call(host.round_div_host, acc, cnt), te8.round_div(acc, cnt))


def test_quantize_multiplier_hand_values():
    from cpx.ml_tools.tflite_graph_i8 import quantize_multiplier

    assert quantize_multiplier(0.5) == (2 ** 30, 0)
    assert quantize_multiplier(1.0) == (2 ** 30, 1)
    assert quantize_multiplier(0.25) == (2 ** 30, -1)
    # f * 2^31 rounds up to 2^31: halved, the exponent one up
    assert quantize_multiplier(1.0 - 2.0 ** -33) == (2 ** 30, 1)
    assert quantize_multiplier(0.0) == (0, 0)
    assert quantize_multiplier(2.0 ** -40) == (0, 0)
    assert quantize_multiplier(2.0 ** -31) == (2 ** 30, -30)
    assert quantize_multiplier(0.75) == (3 * 2 ** 29, 0)
    assert quantize_multiplier(3.0) == te8.quantize_multiplier(3.0) == (3 * 2 ** 29, 2)
