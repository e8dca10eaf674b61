"""The tile walks of conv_block32s_kernel (classifier-pipeline_amd/csrc/cpx_conv_layout_core.h: walk_tile, choose_walk),
compiled for the HOST: the row runs visit every tile exactly once, carry nine tiles in ten at the bench's shape, stay
within one tile row of the mean per workgroup, and the launcher's choice between the two walks is the stated rule.
Needs no GPU; the product never loads this build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "block_walk_host.cpp")
INCLUDES = ["-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc")]
WALK_TILES, WALK_ROWS, CHOSEN = 0, 1, -1
SHAPES = [(1, 1), (2, 2), (3, 3), (10, 10), (10, 3)]  # tiles_x, tiles_y
BATCHES = [1, 3, 7, 1559]
GRIDS = [8, 24, 128]
FIELDS = ("walk", "gx", "total", "visited", "again", "outside", "carried", "most", "least")


def build_host_lib(out):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", *INCLUDES, SRC, "-o", str(out)])
    lib = C.CDLL(str(out))
    lib.block_walk_host.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, C.c_void_p]
    lib.walk_max_tiles_host.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int]
    lib.walk_max_tiles_host.restype = C.c_longlong
    lib.walk_carry_saving_host.restype = C.c_double
    return lib


def walk(lib, tiles_x, tiles_y, n, grid, which=CHOSEN):
    """One launch walked on the host -> dict of FIELDS."""
    out = np.zeros(len(FIELDS), np.int64)
    rc = lib.block_walk_host(tiles_x, tiles_y, n, grid, which, out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return dict(zip(FIELDS, (int(v) for v in out)))


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return build_host_lib(tmp_path_factory.mktemp("block_walk") / "libblock_walk_host.so")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which", [WALK_ROWS, WALK_TILES])
def test_every_tile_exactly_once(host_lib, shape, which):
    tx, ty = shape
    for n in BATCHES:
        for grid in GRIDS:
            w = walk(host_lib, tx, ty, n, grid, which)
            total = tx * ty * n
            assert (w["walk"], w["total"], w["visited"], w["again"], w["outside"]) == (which, total, total, 0, 0), (n, grid, w)
            assert w["gx"] % 8 == 0 and w["gx"] == min(grid, (total + 7) // 8 * 8)
            # balance: the fullest workgroup is within one unit (a tile, or a row of tx tiles) of the mean
            unit = tx if which == WALK_ROWS else 1
            assert w["most"] < total / w["gx"] + unit, (n, grid, w)
            assert w["most"] == host_lib.walk_max_tiles_host(tx, ty, n, which, w["gx"])
            if which == WALK_ROWS:
                # a workgroup walks whole rows right to left: every tile of a row but its first is carried
                assert w["carried"] == (tx - 1) * ty * n, (n, grid, w)
                assert w["most"] % tx == 0 and w["least"] % tx == 0
            else:
                assert w["carried"] == 0, (n, grid, w)  # its tiles ascend: never a left neighbour next


def test_carried_share(host_lib):
    w = walk(host_lib, 10, 10, 1559, 128, WALK_ROWS)
    assert w["carried"] >= 0.89 * w["total"] and w["carried"] == 140310
    assert (w["most"], w["least"]) == (1220, 1210)  # 122 or 121 rows of the 15,590: 0.2 % over the tile walk's 1,218
    assert walk(host_lib, 10, 10, 1559, 128, WALK_TILES)["most"] == 1218
    for n in BATCHES:
        for grid in GRIDS:
            assert walk(host_lib, 1, 1, n, grid, WALK_ROWS)["carried"] == 0
    assert walk(host_lib, 2, 2, 1, 8, WALK_ROWS)["carried"] == 2  # the smallest grid with a carry: one per row


def test_launchers_choice(host_lib):
    """Row runs exactly where their fullest workgroup, a carried tile counted as 1 - saving of a tile, is below the tile
    walk's fullest: the rule restated, and its outcome on the cases that matter."""
    s = host_lib.walk_carry_saving_host()
    assert 0.0 < s < 0.2
    for tx, ty in SHAPES:
        for n in BATCHES:
            for grid in GRIDS:
                got = walk(host_lib, tx, ty, n, grid)
                rows, tiles = (walk(host_lib, tx, ty, n, grid, which)["most"] for which in (WALK_ROWS, WALK_TILES))
                cost = rows / tx * (tx - s * (tx - 1))
                assert got["walk"] == (WALK_ROWS if cost < tiles else WALK_TILES), (tx, ty, n, grid, cost, tiles)
    chosen = lambda tx, ty, n, grid: walk(host_lib, tx, ty, n, grid)["walk"]
    assert chosen(10, 10, 1559, 128) == WALK_ROWS   # the bench's chunk: 1,220 tiles, 1,098 of them carried, against 1,218
    assert chosen(10, 10, 1559, 24) == WALK_ROWS and chosen(10, 10, 1559, 8) == WALK_ROWS
    assert chosen(10, 3, 1559, 128) == WALK_ROWS
    assert chosen(10, 10, 3, 128) == WALK_TILES     # 30 rows on 128 workgroups: 10 tiles against 3
    assert chosen(10, 10, 1, 128) == WALK_TILES and chosen(10, 10, 7, 128) == WALK_TILES
    for n in BATCHES:
        assert chosen(1, 1, n, 128) == WALK_TILES   # nothing to carry: the walks tie, and the tile walk stays
    assert chosen(2, 2, 1, 8) == WALK_TILES         # two rows of two on eight workgroups: one tile each is shorter


def test_standalone_under_sanitizers(tmp_path):
    """The same source as a program of its own (its main walks the same cases and a 4096-wide grid), with ASan + UBSan."""
    exe = tmp_path / "block_walk_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-DBLOCK_WALK_HOST_MAIN", *INCLUDES, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
