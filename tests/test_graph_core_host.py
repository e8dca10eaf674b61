"""The arithmetic and the index maps the graph executor's kernels share (classifier-pipeline_amd/csrc/cpx_graph_core.h and
the host part of cpx_graph_conv_core.h) compiled for the HOST, with -ffp-contract=off as the product, and held bit for bit (float32 viewed as uint32) to the NumPy
restatement of the hybrid arithmetic (tests/tflite_eval_q8.py, which is not translated from the C++) and to divmod.
Needs no GPU; the product never loads this build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tflite_eval_q8 as tq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "graph_core_host.cpp")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc"),
         "-I", os.path.join(REPO, "include")]
RUN = 4   # cpx_graph_dw.hip's GRAPH_DW_RUN, as tests/native/graph_core_host.cpp instantiates the item decomposition
F32, I32 = np.float32, np.int32
ZPS = (-128, -1, 0, 127)
ACTS = (0, 1, 3)   # CPX_GRAPH_ACT_NONE, RELU, RELU6


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("graph_core") / "libgraph_core_host.so"
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *FLAGS, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    u64, i64 = C.c_ulonglong, C.c_longlong
    lib.quads_host.argtypes = [C.c_int, C.c_int, u64, u64]
    lib.conv_pixel_host.argtypes = [i64, i64, C.c_int, C.c_int, C.c_void_p]
    lib.sample_step_host.argtypes = [i64, C.c_int, C.c_int, C.c_void_p]
    lib.dw_item_host.argtypes = [u64, u64, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.conv_geom_host.argtypes = [C.c_int] * 8 + [u64, C.c_void_p]
    lib.conv_step_host.argtypes = [C.c_int] * 4 + [C.c_void_p]
    lib.conv_tiling_host.argtypes = [C.c_int, C.c_void_p]
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    a = np.ascontiguousarray(a, F32)
    return a.view(np.uint32)


# ---- quantise ----
def host_quantise(lib, x, inv, zp):
    x, inv = np.ascontiguousarray(x, F32), np.ascontiguousarray(inv, F32)
    out = np.zeros(x.size, I32)
    lib.quantise_host(ptr(x), ptr(inv), int(zp), x.size, ptr(out))
    return out


def want_quantise(x, inv, zp):
    """tflite_eval_q8.quantise_input takes one inv and zp per sample: every element is a sample of its own."""
    q = tq.quantise_input(np.asarray(x, F32).reshape(-1, 1), np.asarray(inv, F32), np.full(len(x), zp, np.int64))
    return q.reshape(-1).astype(I32)


def quantise_points():
    """(x, inv) whose float32 product is a tie, the float32 on either side of one, beyond both clamps, or a zero."""
    ties = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, 127.5, -128.5], F32)
    prods = np.concatenate([ties, np.nextafter(ties, F32(np.inf)), np.nextafter(ties, F32(-np.inf)),
                            np.array([127.0, 128.0, 300.0, 1e6, -128.0, -129.0, -300.0, -1e6, 0.0, -0.0], F32)])
    xs, invs = [prods], [np.ones_like(prods)]
    for inv in (F32(0.5), F32(2.0), F32(1024.0)):   # powers of two: x * inv is the same product, exactly
        xs.append((prods / inv).astype(F32))
        invs.append(np.full_like(prods, inv))
    # x = 2^-k / 3 rounded, inv = 3 * 2^k ...: products that ROUND onto a tie or next to it in the one float32 multiply
    for inv in (F32(3.0), F32(127.0 / 5.1), F32(255.0 / 7.3)):
        x = (prods.astype(np.float64) / np.float64(inv)).astype(F32)
        xs += [x, np.nextafter(x, F32(np.inf)), np.nextafter(x, F32(-np.inf))]
        invs += [np.full_like(prods, inv)] * 3
    return np.concatenate(xs), np.concatenate(invs)


@pytest.mark.parametrize("zp", ZPS)
def test_quantise_bit_for_bit(lib, zp):
    x, inv = quantise_points()
    prod = (x * inv).astype(F32)
    assert {0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 126.5, 127.5, -128.5} <= set(prod.tolist())   # the ties are really reached
    got, want = host_quantise(lib, x, inv, zp), want_quantise(x, inv, zp)
    assert np.array_equal(got, want), (x[got != want], inv[got != want])
    assert got.min() == -128 and got.max() == 127
    assert host_quantise(lib, [0.0, -0.0], [1.0, 1.0], zp).tolist() == [zp, zp]
    if zp == 0:   # half away from zero, not half to even
        assert host_quantise(lib, [0.5, -0.5, 2.5, -2.5], [1.0] * 4, 0).tolist() == [1, -1, 3, -3]
    rng = np.random.default_rng(1000 + zp)
    x = rng.uniform(-300, 300, size=100000).astype(F32)
    for inv in (F32(1.0), F32(0.5), F32(127.0 / 300.0), F32(255.0 / 431.7), F32(3.3333333), F32(1e-3)):
        inv = np.full_like(x, inv)
        assert np.array_equal(host_quantise(lib, x, inv, zp), want_quantise(x, inv, zp))


# ---- the parameters ----
def host_params(lib, lo, hi, symmetric):
    lo, hi = np.ascontiguousarray(lo, F32), np.ascontiguousarray(hi, F32)
    sx, inv, zp = np.zeros(lo.size, F32), np.zeros(lo.size, F32), np.zeros(lo.size, I32)
    lib.quant_params_host(ptr(lo), ptr(hi), int(symmetric), lo.size, ptr(sx), ptr(inv), ptr(zp))
    return sx, inv, zp


def check_params(lib, lo, hi, symmetric):
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    assert np.all(lo <= 0) and np.all(hi >= 0)   # the kernel's reduction starts from 0: lo = min(0, min x), hi = max(0, max x)
    with np.errstate(over="ignore"):   # (1 / s beyond float32: inf on both sides)
        wsx, winv, wzp = tq.quant_params(np.stack([lo, hi], axis=1), symmetric=symmetric)
    sx, inv, zp = host_params(lib, lo, hi, symmetric)
    assert np.array_equal(bits(sx), bits(wsx)) and np.array_equal(bits(inv), bits(winv)) and np.array_equal(zp, wzp.astype(I32))
    return sx, inv, zp


@pytest.mark.parametrize("symmetric", [False, True], ids=["asymmetric", "symmetric"])
def test_quant_params_bit_for_bit(lib, symmetric):
    sx, inv, zp = check_params(lib, [0.0, -0.0], [0.0, 0.0], symmetric)   # lo == hi == 0
    assert sx.tolist() == [1.0, 1.0] and inv.tolist() == [1.0, 1.0] and zp.tolist() == [0, 0]
    _, _, zp = check_params(lib, [0.0, 0.0, 0.0], [5.0, 255.0, 0.1], symmetric)   # all positive
    assert zp.tolist() == ([0] * 3 if symmetric else [-128] * 3)
    _, _, zp = check_params(lib, [-4.0, -255.0, -0.3], [0.0, 0.0, 0.0], symmetric)   # all negative
    assert zp.tolist() == ([0] * 3 if symmetric else [127] * 3)
    # the candidates cost the same where hi / s + lo / s = 1, i.e. lo = -127 k, hi = 128 k: exactly for a power of two k,
    # within an ulp or two for the others and for the neighbours of hi.  The candidates themselves differ by their
    # rounding alone, which decides zp where they lie next to a half: lo = -127.5 k, hi = 127.5 k.
    ks = np.array([1.0, 0.5, 2.0 ** -20, 2.0 ** 20, 0.1, 0.3, 1.0 / 3.0, 7.7, 1e-3, 12345.678], np.float64)
    for a, b in ((127.0, 128.0), (127.5, 127.5), (126.5, 128.5)):
        lo, hi = (-a * ks).astype(F32), (b * ks).astype(F32)
        los, his = [lo] * 5, [hi]
        for d in (np.inf, -np.inf):
            his += [np.nextafter(hi, F32(d)), np.nextafter(np.nextafter(hi, F32(d)), F32(d))]
        _, _, zp = check_params(lib, np.concatenate(los), np.concatenate(his), symmetric)
        if not symmetric:
            assert set(zp.tolist()) <= {-3, -2, -1, 0} and (a != 127.0 or zp[0] == -1)
    tiny = np.array([1e-45, 3e-45, 1e-40, 1.1754942e-38], F32)   # hi - lo denormal
    check_params(lib, np.concatenate([-tiny, 0 * tiny, -tiny]), np.concatenate([0 * tiny, tiny, tiny]), symmetric)
    big = np.array([3.4028235e38, 3.4e38, 1.7014118e38, 1e38], F32)   # hi - lo near (and, in float64, beyond) float32's largest
    check_params(lib, np.concatenate([-big, 0 * big, -big, -tiny]), np.concatenate([0 * big, big, big, big]), symmetric)
    rng = np.random.default_rng(77 + symmetric)
    lo = -np.abs(rng.normal(0, 1, size=10000) * 10.0 ** rng.uniform(-6, 6, size=10000))
    hi = np.abs(rng.normal(0, 1, size=10000) * 10.0 ** rng.uniform(-6, 6, size=10000))
    lo[::7], hi[3::11] = 0.0, 0.0
    check_params(lib, lo, hi, symmetric)


# ---- the finish ----
def host_finish(lib, acc, zp, wsum, sx, scale, shift, act):
    arrs = [np.ascontiguousarray(a, I32) for a in (acc, zp, wsum)] + [np.ascontiguousarray(a, F32) for a in (sx, scale, shift)]
    out = np.zeros(arrs[0].size, F32)
    lib.hybrid_finish_host(*[ptr(a) for a in arrs], int(act), out.size, ptr(out))
    return out


def check_finish(lib, acc, zp, wsum, sx, scale, shift, act):
    """tflite_eval_q8._finish takes acc - zp * wsum as float64 integers [sample, channel], sx per sample, scale and shift
    per channel: every element is a sample of its own, and the elements of one (scale, shift) are one channel."""
    acc, zp, wsum = (np.asarray(a, np.int64) for a in (acc, zp, wsum))
    acc_z = (acc - zp * wsum).astype(np.float64)
    assert np.all(np.abs(acc_z) < 2 ** 31) and np.all(np.abs(zp * wsum) < 2 ** 31)
    got = host_finish(lib, acc, zp, wsum, sx, scale, shift, act)
    for sc, sf in sorted(set(zip(np.asarray(scale, F32).tolist(), np.asarray(shift, F32).tolist()))):
        pick = (np.asarray(scale, F32) == F32(sc)) & (np.asarray(shift, F32) == F32(sf))
        want, _ = tq._finish(acc_z[pick].reshape(-1, 1), np.asarray(sx, F32)[pick], np.array([sc], F32), np.array([sf], F32), act)
        assert np.array_equal(bits(got[pick]), bits(want.reshape(-1))), (sc, sf, act)
    return got


@pytest.mark.parametrize("act", ACTS)
def test_hybrid_finish_bit_for_bit(lib, act):
    K = (2 ** 31 - 1) // (127 * 255)   # the most products the planner's overflow check lets through
    assert K * 127 * 255 < 2 ** 31 <= (K + 1) * 127 * 255
    # (acc, zp, wsum): acc - zp * wsum at 0 and +-1, at +-(2^24 + 1), at the largest magnitude of either sign
    cases = [(0, 0, 0), (-128 * 77, -128, 77), (127 * 5, 127, 5), (1, 0, 0), (-1, 0, 0), (127 * 9 + 1, 127, 9), (-128 * 9 - 1, -128, 9),
             (2 ** 24 + 1, 0, 0), (-(2 ** 24 + 1), 0, 0), (2 ** 24 + 1 - 128 * 1000, -128, 1000), (-(2 ** 24 + 1) + 127 * 1000, 127, 1000),
             (2 ** 24 + 3, 0, 0), (K * 127 * 127, -128, K * 127), (-K * 127 * 127, -128, -K * 127), (-K * 128 * 127, 127, K * 127)]
    consts = [(1.0, 1.0, 0.0), (0.0123, 0.0071, -0.3), (3.7e-3, 1.9e-2, 2.5), (1e-6, 1e-3, 1e-7), (0.25, 0.5, -1e-3)]
    acc, zp, wsum, sx, scale, shift = ([] for _ in range(6))
    for a, z, w in cases:
        for s, c, f in consts:
            acc.append(a), zp.append(z), wsum.append(w), sx.append(s), scale.append(c), shift.append(f)
    got = check_finish(lib, acc, zp, wsum, sx, scale, shift, act)
    n = len(consts)
    assert got[0] == 0.0 and got[3 * n] == 1.0 and got[4 * n] == (-1.0 if act == 0 else 0.0)
    assert got[7 * n] == (2.0 ** 24 if act != 3 else 6.0)   # 2^24 + 1 rounds to even in the conversion
    assert got[12 * n] == (float(F32(K * 127 * 255)) if act != 3 else 6.0)
    rng = np.random.default_rng(500 + act)
    m = 20000
    zp, wsum = rng.integers(-128, 128, size=m), rng.integers(-127 * 4096, 127 * 4096 + 1, size=m)
    acc_z = rng.integers(-K * 127 * 255, K * 127 * 255 + 1, size=m)
    acc_z[::3] = rng.integers(-70000, 70001, size=len(acc_z[::3]))   # where activations and shifts decide the value
    acc = np.clip(acc_z + zp * wsum, -2 ** 31, 2 ** 31 - 1)
    sx = (10.0 ** rng.uniform(-4, 0, size=m)).astype(F32)
    pairs = [(F32(10.0 ** rng.uniform(-4, -1)), F32(rng.normal(0, 1))) for _ in range(8)]
    which = rng.integers(0, 8, size=m)
    check_finish(lib, acc, zp, wsum, sx, [pairs[k][0] for k in which], [pairs[k][1] for k in which], act)


# ---- the view predicate ----
def test_quads_predicate(lib):
    assert lib.quads_host(8, 8, 64, 4096) == 1 and lib.quads_host(4, 12, 12 * 49, 16) == 1
    assert lib.quads_host(6, 8, 64, 4096) == 0      # C
    assert lib.quads_host(8, 10, 64, 4096) == 0     # the row stride
    assert lib.quads_host(8, 8, 66, 4096) == 0      # the sample stride
    for off in (4, 8, 12):                          # a slice at a channel that is no multiple of 4
        assert lib.quads_host(8, 8, 64, 4096 + off) == 0


# ---- the flattened pixels of CONV / CONV_Q8 ----
MAPS = [(1, 1), (3, 3), (3, 1), (64, 8), (289, 17)]   # HoWo, Wo


@pytest.mark.parametrize("howo,wo", MAPS)
def test_conv_pixel_and_epilogue_step(lib, howo, wo):
    out = np.zeros(4, np.int64)
    for n_samples in (1, 2, 300 // howo + 2):   # tiles of 128 pixels straddle one boundary and several (HoWo = 1: 127)
        P = n_samples * howo
        tiles = -(-P // 128)
        for p in range(tiles * 128):
            lib.conv_pixel_host(p, P, howo, wo, ptr(out))
            if p < P:
                n, rem = divmod(p, howo)
                assert out.tolist() == [n, *divmod(rem, wo), 1], (p, P)
            else:
                assert out.tolist() == [0, 0, 0, 0], (p, P)
        # the epilogue: a wave's 32 rows from its first pixel's (sample, pixel)
        for pb in range(0, tiles * 128, 32):
            if pb >= P:
                continue
            nb, remb = divmod(pb, howo)
            for i in range(32):
                lib.sample_step_host(nb, remb + i, howo, ptr(out))
                assert out[:2].tolist() == list(divmod(pb + i, howo)), (pb, i)
    if howo == 1:
        lib.sample_step_host(5, 127, 1, ptr(out))
        assert out[:2].tolist() == [132, 0]
    # a batch beyond 2^31 pixels
    P = 2 ** 33 + 5
    lib.conv_pixel_host(P - 1, P, howo, wo, ptr(out))
    n, rem = divmod(P - 1, howo)
    assert out.tolist() == [n, *divmod(rem, wo), 1]
    for o, stride, pad in [(0, 1, 0), (0, 2, 1), (5, 2, 3), (16, 1, 6)]:
        assert lib.window_origin_host(o, stride, pad) == o * stride - pad


def test_accumulator_row_map_is_a_permutation(lib):
    rows = [lib.acc_row_host(r, lane) for lane in (0, 32) for r in range(16)]
    assert sorted(rows) == list(range(32))
    for lane in range(256):   # only bit 5 matters, of a lane or of a thread's index; a register quad is four consecutive rows
        assert [lib.acc_row_host(r, lane) for r in range(16)] == [lib.acc_row_host(r, lane & 32) for r in range(16)]
    assert [lib.acc_row_host(r, 0) for r in range(8)] == [0, 1, 2, 3, 8, 9, 10, 11] and lib.acc_row_host(0, 32) == 4


# ---- the convolutions' launch geometry, K steps and tiles (cpx_graph_conv_core.h) ----
def around(m):
    """one below, at and one above a multiple of m, and m's neighbourhood itself"""
    return sorted({v for k in (1, 3) for v in (k * m - 1, k * m, k * m + 1) if v >= 1})


@pytest.mark.parametrize("kc", [16, 32])
@pytest.mark.parametrize("groups", [1, 2, 3])
def test_conv_geometry_is_plain_arithmetic(lib, groups, kc):
    """P, HoWo, the group's channels, its chunks of kc input channels and tiles of 32 output channels, and the 16-byte
    test of either element type, over Cin and Cout per group around the multiples of the chunk and the tile."""
    out = np.zeros(8, np.int64)
    N, Ho, Wo = 3, 5, 4
    for cg in around(kc) + [4, 8, 20]:
        for cog in around(32):
            cin, cout = groups * cg, groups * cog
            for as_bytes, address in ((0, 4096), (1, 4096), (0, 4096 + 4), (1, 4096 + 8)):
                lib.conv_geom_host(N, Ho, Wo, cin, cout, kc, groups, as_bytes, address, ptr(out))
                # (the views are dense: row stride Cin, sample stride 49 Cin, so the strides are aligned where Cin is)
                lanes = 16 if as_bytes else 4
                vec = cg % lanes == 0 and cin % lanes == 0 and address % 16 == 0
                want = [N * Ho * Wo, Ho * Wo, -(-cg // kc), -(-cog // 32), int(vec), cg, cog, groups]
                assert out.tolist() == want, (cin, cout, groups, kc, as_bytes, address)


@pytest.mark.parametrize("nchunks", [1, 2, 5])
@pytest.mark.parametrize("kw", [1, 3, 7])
@pytest.mark.parametrize("kh", [1, 3, 7])
def test_conv_step_is_divmod(lib, kh, kw, nchunks):
    out = np.zeros(4, I32)
    for kc in (16, 32):
        for s in range(kh * kw * nchunks):
            lib.conv_step_host(s, nchunks, kw, kc, ptr(out))
            tap, chunk = divmod(s, nchunks)
            assert out.tolist() == [tap, chunk * kc, *divmod(tap, kw)], (s, kc)
            assert 0 <= out[2] < kh


def test_conv_tiles_per_wave_and_grid_rows(lib):
    out = np.zeros(2, I32)
    table = {1: (1, 1), 2: (2, 1), 3: (4, 1), 4: (4, 1), 5: (4, 2), 9: (4, 3)}
    for ntiles, want in table.items():
        lib.conv_tiling_host(ntiles, ptr(out))
        assert tuple(out.tolist()) == want, ntiles
    for ntiles in range(1, 70):   # every tile is some wave's: NTN * rows covers them, with less than a row to spare
        lib.conv_tiling_host(ntiles, ptr(out))
        assert out[0] in (1, 2, 4) and out[0] * (out[1] - 1) < ntiles <= out[0] * out[1]


# ---- the depthwise work item ----
def want_item(idx, groups, runs, ho):
    t, g = divmod(idx, groups)
    u, run = divmod(t, runs)
    n, oy = divmod(u, ho)
    return [n, oy, RUN * run, 4 * g]


def host_item(lib, idx, items, groups, runs, ho):
    """items < 2^32: the 32-bit divisions; from 2^32 on the 64-bit ones, whatever idx is"""
    out = np.zeros(4, np.uint64)
    ok = lib.dw_item_host(idx, items, groups, runs, ho, ptr(out))
    return ok, [int(v) for v in out]


def test_depthwise_item_both_paths_below_2_32(lib):
    rng = np.random.default_rng(3)
    for groups, runs, ho, n in [(1, 1, 1, 3), (5, 3, 9, 7), (36, 2, 7, 5), (48, 28, 112, 6), (1, 1, 1, 2 ** 32 - 1), (240, 4, 14, 300000)]:
        items = n * ho * runs * groups
        assert items < 2 ** 32
        idxs = set(range(min(items, 1000))) | {items - 1, items // 2} | set(int(v) for v in rng.integers(0, items, size=300))
        for idx in sorted(idxs):
            want = want_item(idx, groups, runs, ho)
            assert host_item(lib, idx, items, groups, runs, ho) == (1, want)
            assert host_item(lib, idx, items + 2 ** 32, groups, runs, ho) == (1, want)   # the 64-bit path on the same item
        assert host_item(lib, items, items, groups, runs, ho)[0] == 0   # beyond the last item
        assert host_item(lib, items + 255, items, groups, runs, ho)[0] == 0


def test_depthwise_item_64_bit_path(lib):
    """Item counts and indices above 2^32: what no GPU test of a few seconds reaches."""
    rng = np.random.default_rng(4)
    for groups, runs, ho in [(48, 28, 112), (1, 1, 1), (240, 4, 14), (3, 2, 5)]:
        per = ho * runs * groups
        for items in (2 ** 32, 2 ** 32 + per, -(-2 ** 36 // per) * per, -(-2 ** 44 // per) * per):
            idxs = {0, 1, per - 1, per, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, items - 1} | set(int(v) for v in rng.integers(0, items, size=200))
            for idx in sorted(i for i in idxs if i < items):
                want = want_item(idx, groups, runs, ho)
                assert want[0] < 2 ** 63
                assert host_item(lib, idx, items, groups, runs, ho) == (1, want), (idx, items)
            assert host_item(lib, items, items, groups, runs, ho)[0] == 0


def test_standalone_under_sanitizers(tmp_path):
    """The same source as a program of its own (its main walks the same ground), built with ASan + UBSan."""
    exe = tmp_path / "graph_core_host"
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-DGRAPH_CORE_HOST_MAIN", *FLAGS, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
