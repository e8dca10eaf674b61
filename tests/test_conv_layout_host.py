"""The convolution launchers' host knowledge (classifier-pipeline_amd/csrc/cpx_conv_layout_core.h: a layer's class, the
layout of its weight-image buffer, the tile decomposition's multipliers and range, the persistent grid width) compiled
for the HOST and checked against the layout table restated here in Python, not translated from the C++.  Needs no GPU;
the product never loads this build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "conv_layout_host.cpp")
INCLUDES = ["-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc")]
CLASSES = ("Unsupported", "Plain", "Flat", "Wide", "C8", "Stride2Rw", "Rw3")  # ConvClass's order
IMAGES = ("planes3", "planes2", "half", "scales", "rw_half")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("conv_layout") / "libconv_layout_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", *INCLUDES, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.tile_magic_host.restype = C.c_uint64
    lib.tile_fill_host.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    lib.persistent_grid_x_host.argtypes = [C.c_int, C.c_int, C.c_longlong]
    lib.persistent_grid_host.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_char_p]
    return lib


def host_layout(lib, cin, cout, groups, ksize=3, stride=1):
    """-> (class name, {image: offset} of the images that exist, total bytes, conv_rw_kind)"""
    out = np.zeros(8, np.int64)
    kind = lib.conv_layout_host(cin, cout, groups, ksize, stride, out.ctypes.data_as(C.c_void_p))
    offs = {name: int(v) for name, v in zip(IMAGES, out[2:7]) if v >= 0}
    return CLASSES[out[0]], offs, int(out[7]), kind


def table_layout(cin, cout, groups, ksize=3, stride=1):
    """The issue's table: -> (class name, [(image, bytes)] in buffer order).  A row is cout_g entries of 16 bytes; an image
    in chunks of c input channels is groups * cin_g / c chunks of so many rows."""
    cin_g, cout_g = cin // groups, cout // groups
    row = 16 * cout_g
    scales = ("scales", -(-2 * cout * 4 // 16) * 16)
    chunks = lambda c, rows: groups * (cin_g // c) * rows * row
    sixteens = cin_g >= 16 and cin_g % 16 == 0
    if ksize != 3 or cin % groups or cout % groups:
        return "Unsupported", []
    if stride == 3 and (cin_g, cout_g) == (64, 128):
        return "Rw3", [("half", chunks(32, 72)), scales]
    if stride == 2 and (cin_g, cout_g) == (32, 64):
        return "Stride2Rw", [("planes3", chunks(16, 54)), ("planes2", chunks(16, 36)), ("half", chunks(16, 36)), scales,
                             ("rw_half", chunks(32, 72))]
    if stride == 1 and (cin_g, cout_g) == (8, 32):
        return "C8", [("planes3", groups * 30 * row), ("half", groups * (3 * 2 * 4 * 32) * 16), scales]
    if stride == 1 and cin_g in (32, 64) and cout_g in (32, 64):
        return "Wide", [("planes3", chunks(32, 108)), ("planes2", chunks(32, 72)), ("half", chunks(32, 72)), scales]
    if sixteens and ((stride == 1 and cout_g == 128) or (stride == 2 and cout_g == 64)):
        return "Flat", [("planes3", chunks(16, 54)), ("planes2", chunks(16, 36)), ("half", chunks(16, 36)), scales]
    if sixteens and stride == 1 and cout_g in (32, 64):
        return "Plain", [("planes3", chunks(16, 54))]
    return "Unsupported", []


def offsets_of(images):
    offs, at = {}, 0
    for name, size in images:
        offs[name] = at
        at += size
    return offs, at


# (Cin, Cout, stride) at groups = 2 -> class, offsets in buffer order, total: the issue's worked values
WORKED = [
    ((16, 64, 1), "C8", {"planes3": 0, "half": 30720, "scales": 55296}, 55808),
    ((64, 64, 1), "Wide", {"planes3": 0, "planes2": 110592, "half": 184320, "scales": 258048}, 258560),
    ((64, 128, 2), "Stride2Rw", {"planes3": 0, "planes2": 221184, "half": 368640, "scales": 516096, "rw_half": 517120}, 664576),
    ((128, 128, 1), "Wide", {"planes3": 0, "planes2": 442368, "half": 737280, "scales": 1032192}, 1033216),
    ((128, 256, 3), "Rw3", {"half": 0, "scales": 589824}, 591872),
    ((256, 256, 1), "Flat", {"planes3": 0, "planes2": 1769472, "half": 2949120, "scales": 4128768}, 4130816),
    ((32, 64, 1), "Plain", {"planes3": 0}, 55296),
]
# one shape of each class as channels per group (in, out, stride), and shapes next to the classes' edges
PER_GROUP = [(8, 32, 1), (32, 32, 1), (32, 64, 2), (64, 64, 1), (64, 128, 3), (128, 128, 1), (16, 32, 1), (16, 64, 2),
             (128, 64, 1), (32, 64, 1), (64, 32, 1), (64, 128, 1), (48, 64, 1), (96, 128, 1), (24, 32, 1), (8, 32, 2),
             (8, 64, 1), (16, 32, 2), (64, 128, 2), (32, 64, 3), (16, 16, 1), (64, 256, 1)]


@pytest.mark.parametrize("shape,cls,offs,total", WORKED)
def test_worked_values(host_lib, shape, cls, offs, total):
    cin, cout, stride = shape
    want_cls, images = table_layout(cin, cout, 2, 3, stride)
    assert (want_cls, *offsets_of(images)) == (cls, offs, total)  # the restatement against the worked values
    assert host_layout(host_lib, cin, cout, 2, 3, stride)[:3] == (cls, offs, total)


def test_classes_by_name(host_lib):
    cls = lambda cin, cout, stride=1, ksize=3: host_layout(host_lib, cin, cout, 2, ksize, stride)
    assert cls(32, 128, 2)[0] == "Flat" and "rw_half" not in cls(32, 128, 2)[1]
    assert cls(256, 128)[0] == "Plain"
    assert cls(64, 128)[0] == "Wide" and cls(128, 64)[0] == "Wide"
    assert cls(48, 64) == ("Unsupported", {}, 0, 0)  # cin_g = 24
    for cin, cout, stride in [(16, 64, 1), (64, 64, 1), (64, 128, 2), (128, 256, 3), (256, 256, 1)]:
        assert cls(cin, cout, stride, 5) == ("Unsupported", {}, 0, 0)
    assert host_layout(host_lib, 17, 64, 2)[0] == "Unsupported"  # channels that do not divide into the groups


@pytest.mark.parametrize("groups", [1, 2, 4])
def test_layout_matches_table(host_lib, groups):
    seen = set()
    for cin_g, cout_g, stride in PER_GROUP:
        cin, cout = cin_g * groups, cout_g * groups
        want_cls, images = table_layout(cin, cout, groups, 3, stride)
        want_offs, want_total = offsets_of(images)
        cls, offs, total, kind = host_layout(host_lib, cin, cout, groups, 3, stride)
        assert (cls, offs, total) == (want_cls, want_offs, want_total), (cin_g, cout_g, stride)
        seen.add(cls)
        # in the stated order, disjoint, 16-byte aligned, back to back, the last one ending at `bytes`
        at = 0
        for name, size in images:
            assert offs[name] == at and at % 16 == 0 and size > 0
            at += size
        assert at == total
        want_kind = {"Rw3": 3, "Stride2Rw": 2}.get(cls, 1 if cls == "Wide" and (cin_g, cout_g) == (64, 64) else 0)
        assert kind == want_kind, (cin_g, cout_g, stride)
    assert seen == set(CLASSES)


def test_tile_magic_exact_to_the_edge_of_its_range(host_lib):
    for d in (1, 2, 3, 7, 8, 4095):
        m = int(host_lib.tile_magic_host(d))
        ns = {0, d - 1, d, d + 1, 2 ** 22 - 1}
        for k in (2, 3, 1000, (2 ** 22 - 1) // d):
            ns |= {k * d - 1, k * d}
        for n in ns:
            assert 0 <= n < 2 ** 22
            assert n * m < 2 ** 64 and (n * m) >> 42 == n // d, (n, d)  # (n * m < 2^64: what the device's 64-bit product holds)


def test_tile_div_at_the_edges_of_its_range(host_lib):
    """The one division the kernels and the block walk share (tile_div), at the largest index a persistent grid forms
    (2^22 - 9, + 7 for the walk's rounding) and the largest count along an axis (4095)."""
    div = host_lib.tile_div_host
    for d in (1, 2, 3, 7, 10, 4094, 4095):
        for n in (0, d - 1, d, min(4095 * d, 2 ** 22) - 1, 2 ** 22 - 9, 2 ** 22 - 2, 2 ** 22 - 1):
            assert 0 <= n < 2 ** 22 and div(n, d) == n // d, (n, d)
    assert div(2 ** 22 - 9, 4095) == 1024


def fill(lib, tx, ty, n, nsplit=0, persistent=0):
    out = np.zeros(7, np.uint64)
    rc = lib.tile_fill_host(tx, ty, n, nsplit, persistent, out.ctypes.data_as(C.c_void_p))
    return rc, [int(v) for v in out]


def test_tile_filler_fields_and_range_errors(host_lib):
    rc, (m_ns, m_tx, m_ty, nsplit, tx, ty, total) = fill(host_lib, 10, 7, 3, nsplit=2)
    assert rc == 0 and (nsplit, tx, ty, total) == (2, 10, 7, 10 * 7 * 3 * 2)
    assert (m_ns, m_tx, m_ty) == (2 ** 42 // 2 + 1, 2 ** 42 // 10 + 1, 2 ** 42 // 7 + 1)
    rc, (m_ns, m_tx, m_ty, nsplit, tx, ty, total) = fill(host_lib, 5, 1, 4)  # the form without a column split
    assert rc == 0 and (m_ns, nsplit, m_ty, total) == (0, 0, 2 ** 42 + 1, 20)
    # 2^22 units of work for the one-per-workgroup launches, 2^22 - 8 tiles for the persistent ones, 4096 along an axis
    assert fill(host_lib, 2048, 1024, 1, nsplit=2)[0] == -3 and fill(host_lib, 2048, 2048, 1)[0] == -3
    rc, out = fill(host_lib, 2048 * 2 - 1, 1, 512, nsplit=2)
    assert rc == 0 and out[6] == 2 ** 22 - 1024
    rc, out = fill(host_lib, 1, 1, 2 ** 22 - 1)
    assert rc == 0 and out[6] == 2 ** 22 - 1
    assert fill(host_lib, 1, 1, 2 ** 22 - 8, persistent=1)[0] == -3
    rc, out = fill(host_lib, 1, 1, 2 ** 22 - 9, persistent=1)
    assert rc == 0 and out[6] == 2 ** 22 - 9
    for persistent in (0, 1):
        assert fill(host_lib, 4096, 1, 1, persistent=persistent)[0] == -3
        assert fill(host_lib, 1, 4096, 1, persistent=persistent)[0] == -3
        assert fill(host_lib, 4095, 1, 1, persistent=persistent)[0] == 0
        assert fill(host_lib, 1, 4095, 1, persistent=persistent)[0] == 0


def test_persistent_grid_x(host_lib):
    gx = host_lib.persistent_grid_x_host
    assert (gx(256, 2, 10 ** 6), gx(256, 4, 10 ** 6), gx(256, 64, 10 ** 6)) == (128, 64, 8)
    for cus in (8, 60, 104, 256, 304):
        for ny in (1, 2, 3, 4, 8, 64):
            for tiles in (1, 7, 8, 9, 63, 64, 65, 1000, 2 ** 22 - 9):
                g = gx(cus, ny, tiles)
                assert g % 8 == 0 and g >= 8 and g <= (tiles + 7) // 8 * 8
                assert g == min(max(8, cus // ny // 8 * 8), (tiles + 7) // 8 * 8)


def test_persistent_grid_width_and_its_override(host_lib, monkeypatch):
    """persistent_grid: persistent_grid_x on the device's CUs shared among the rows; -1 without a device; where the named
    variable is set, its value as the CUs of the whole grid (what CPX_BLOCK32_GRID means to the block launchers)."""
    pg = host_lib.persistent_grid_host
    monkeypatch.delenv("CPX_TEST_GRID", raising=False)
    assert pg(256, 2, 10 ** 6, None) == 128 and pg(256, 2, 10 ** 6, b"CPX_TEST_GRID") == 128
    assert pg(0, 2, 10 ** 6, None) == -1 and pg(256, 2, 9, None) == 16
    monkeypatch.setenv("CPX_TEST_GRID", "64")
    assert pg(256, 2, 10 ** 6, b"CPX_TEST_GRID") == 64 and pg(256, 2, 10 ** 6, None) == 128
    assert pg(256, 2, 9, b"CPX_TEST_GRID") == 16 and pg(0, 2, 10 ** 6, b"CPX_TEST_GRID") == -1


def test_standalone_under_sanitizers(tmp_path):
    """The same source as a program of its own (its main sweeps shapes, multipliers and limits), built with ASan + UBSan."""
    exe = tmp_path / "conv_layout_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-DCONV_LAYOUT_HOST_MAIN", *INCLUDES, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
