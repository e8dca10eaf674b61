"""The geometry of a flattened band (classifier-pipeline_amd/csrc/cpx_flat_band_core.h: a band's rows, its staged pixels, a
staging item's pixel, the patch offset of a position and tap) compiled for the HOST.  conv_flat16_kernel addresses its patch
buffer with these functions and flat_pays's capacity test is flat_band_max_pixels, so what holds here holds for every LDS
address the kernel forms.  Needs no GPU; the product never loads this build.

The sweep covers every H x W in 1..64 x 1..64 whose bands fit the 256-pixel buffer -- a superset of what flat_pays admits
(it also asks that the flattened tiling pays over the rectangular bands).

One property is stated more narrowly than "every staged pixel of an interior band is read by some position": the bands stage
FULL rows, so the first staged row holds pixels left of the first position's window and the last staged row pixels right
of the last position's, which nothing reads (27 x 27, band 1 starts at row 4, column 20: row 3's columns 0..18).  The test
requires that in every band with all 128 positions inside the map the unread pixels lie in these two runs and nowhere else."""
import ctypes as C
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "flat_band_host.cpp")
INCLUDES = ["-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc")]
BAND, CAP = 128, 256  # conv_flat16_kernel's (and conv_bf3flat_kernel's) band and patch capacity
PROPERTY = {1: "staged pixels <= capacity", 2: "(position, tap) offset inside the staged pixels",
            3: "offset names the input pixel the tap reads", 4: "unread staged pixels are the two row-end runs",
            5: "bands tile the positions"}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("flat_band") / "libflat_band_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", *INCLUDES, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.flat_band_host.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    lib.flat_item_pixel_host.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] * 2
    return lib


def band_of(lib, ti, H, W):
    out = (C.c_int * 6)()
    lib.flat_band_host(ti, BAND, H, W, out)
    return dict(zip(("p0", "y_first", "y_last", "PW", "PH", "npx"), out))


def fits(W):
    """a band of 128 positions that starts on a row's last position touches the most rows; + a halo row and column each side"""
    rows = 1 + -(-(BAND - 1) // W)
    return (rows + 2) * (W + 2) <= CAP


def test_capacity_is_the_restated_rule(host_lib):
    for W in range(1, 65):
        assert (host_lib.flat_band_max_pixels_host(BAND, W) <= CAP) == fits(W), W
    assert fits(30) and not fits(31)  # the widest row the 256-pixel patch admits: 8 rows x 32 pixels


def test_sweep_every_map_the_capacity_admits(host_lib):
    maps = 0
    for W in range(1, 65):
        for H in range(1, 65):
            rc = host_lib.flat_sweep_host(H, W, BAND, CAP)
            if fits(W):
                assert rc == 0, (H, W, PROPERTY[rc])
                maps += 1
            else:
                assert rc == 1, (H, W)
    assert maps == 64 * sum(fits(W) for W in range(1, 65)) and maps >= 64 * 30


@pytest.mark.parametrize("H,W", [(27, 27), (9, 11), (13, 13), (13, 29), (13, 30), (50, 3), (1, 1), (64, 30)])
def test_bands_restated_in_python(host_lib, H, W):
    """Independently of the header: the rows a band touches, from its positions; each (position, tap) offset leads, through
    the item -> pixel map, to the input pixel the convolution reads; all offsets inside the staged pixels."""
    M = H * W
    assert host_lib.flat_bands_host(BAND, H, W) == -(-M // BAND)
    for ti in range(-(-M // BAND)):
        b = band_of(host_lib, ti, H, W)
        pos = range(ti * BAND, min(ti * BAND + BAND, M))
        rows = [p // W for p in pos]
        assert (b["p0"], b["y_first"], b["y_last"]) == (pos[0], rows[0], rows[-1])
        assert (b["PW"], b["PH"], b["npx"]) == (W + 2, rows[-1] - rows[0] + 3, (W + 2) * (rows[-1] - rows[0] + 3))
        assert b["npx"] <= CAP
        iy, ix = C.c_int(), C.c_int()
        for p in list(pos)[:: max(1, len(pos) // 16)] + [pos[-1], ti * BAND + BAND - 1]:  # (the last: clamped when past the map)
            pc = min(p, M - 1)
            for ky in range(3):
                for kx in range(3):
                    off = host_lib.flat_patch_offset_host(ti, BAND, H, W, p, ky, kx)
                    assert 0 <= off < b["npx"]
                    host_lib.flat_item_pixel_host(ti, BAND, H, W, off, C.byref(iy), C.byref(ix))
                    assert (iy.value, ix.value) == (pc // W - 1 + ky, pc % W - 1 + kx)


def test_sweep_reports_a_broken_capacity(host_lib):
    assert host_lib.flat_sweep_host(27, 27, BAND, 231) == 1  # a band of 27 x 27 stages 8 x 29 = 232 pixels
    assert host_lib.flat_sweep_host(27, 27, BAND, 232) == 0


def test_standalone_under_sanitizers(tmp_path):
    """The same source as a program of its own (its main sweeps every admitted map), built with ASan + UBSan."""
    exe = tmp_path / "flat_band_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-DFLAT_BAND_HOST_MAIN", *INCLUDES, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
