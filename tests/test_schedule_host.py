"""The frame schedule (classifier-pipeline_amd/csrc/cpx_schedule_core.h: which frames are processed, their FFC flags,
the clip order, the flat layout the device reads) compiled for the HOST and checked against a few lines of NumPy
written from the rules, not from the C++.  Needs no GPU; the product never loads this build."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "schedule_host.cpp")
INCLUDES = ["-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "classifier-pipeline_amd", "csrc")]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("schedule") / "libschedule_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", *INCLUDES, SRC, "-o", str(out)])
    return C.CDLL(str(out))


def make_meta(background, has_times=None, time_on=None, last_ffc=None):
    from cpx._lib import FRAME_META_DTYPE

    m = np.zeros(len(background), FRAME_META_DTYPE)
    m["background_frame"] = background
    if has_times is not None:
        m["has_times"], m["time_on_ms"], m["last_ffc_ms"] = has_times, time_on, last_ffc
    return m


def run_host(host_lib, offs, meta, max_frames):
    """-> (status, flat, layout dict, total, max_proc); flat and layout are None unless status == 0."""
    offs = np.ascontiguousarray(offs, np.int32)
    B = len(offs) - 1
    flat = np.full(3 * B + 3 + 2 * len(meta), -7, np.int32)
    layout = np.zeros(6, np.int64)
    tm = np.zeros(2, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = host_lib.schedule_host(p(offs), p(meta), B, max_frames, p(flat), len(flat), p(layout), p(tm))
    if rc != 0:
        return rc, None, None, 0, 0
    names = ("clip_first", "proc_off", "proc_idx", "proc_ffc", "order", "ints")
    lay = dict(zip(names, (int(v) for v in layout)))
    assert np.all(flat[lay["ints"]:] == -7)  # nothing written past the layout's end
    return rc, flat[:lay["ints"]], lay, int(tm[0]), int(tm[1])


def numpy_schedule(offs, meta):
    """The flat array from the rules: processed = not a background frame; FFC = times known and fewer than 9 ms since
    the last FFC; clips by falling processed length, ties in index order; proc_idx / proc_ffc padded to one int."""
    offs = np.asarray(offs)
    B = len(offs) - 1
    proc = np.flatnonzero(meta["background_frame"] == 0)
    ffc = ((meta["has_times"] != 0) & (meta["time_on_ms"] - meta["last_ffc_ms"] < 9)).astype(np.int32)[proc]
    proc_off = np.searchsorted(proc, offs)  # processed frames in front of each clip boundary
    order = np.argsort(-np.diff(proc_off), kind="stable")
    n = max(len(proc), 1)
    pad = lambda a: np.concatenate([a, np.zeros(n - len(a), np.int64)])
    flat = np.concatenate([offs[:-1], proc_off, pad(proc), pad(ffc), order]).astype(np.int32)
    lay = {"clip_first": 0, "proc_off": B, "proc_idx": 2 * B + 1, "proc_ffc": 2 * B + 1 + n, "order": 2 * B + 1 + 2 * n,
           "ints": 3 * B + 1 + 2 * n}
    return flat, lay, int(np.diff(proc_off).max())


def check(host_lib, offs, meta, max_frames):
    rc, flat, lay, total, max_proc = run_host(host_lib, offs, meta, max_frames)
    assert rc == 0
    want, want_lay, want_max = numpy_schedule(offs, meta)
    assert lay == want_lay
    assert np.array_equal(flat, want)
    assert (total, max_proc) == (offs[-1], want_max)
    return flat, lay


def test_no_processed_frames(host_lib):
    flat, lay = check(host_lib, [0, 3], make_meta([1, 1, 1]), 10)
    B = 1
    assert lay["ints"] == B + (B + 1) + 2 + B
    assert flat[lay["proc_idx"]] == 0 and flat[lay["proc_ffc"]] == 0  # the two padding ints


def test_ffc_boundary(host_lib):
    on = np.array([1008, 1009, 1008, 1009, 5])
    for has_times, want in ((1, [1, 0, 1, 0, 1]), (0, [0, 0, 0, 0, 0])):
        meta = make_meta([0] * 5, has_times, on, 1000)
        flat, lay = check(host_lib, [0, 5], meta, 10)
        assert list(flat[lay["proc_ffc"]:lay["order"]]) == want


def test_order_longest_first_ties_by_index(host_lib):
    bg = []
    offs = [0]
    for n in (3, 7, 3, 7, 1):  # a background frame in front of each clip: frame indices differ from step indices
        bg += [1] + [0] * n
        offs.append(len(bg))
    flat, lay = check(host_lib, offs, make_meta(bg), 7)
    assert list(flat[lay["order"]:]) == [1, 3, 0, 2, 4]


def test_too_long_counts_processed_frames_only(host_lib):
    max_frames = 6
    bg = [1, 0, 0, 0, 1, 0, 0, 0]  # max_frames processed + two background frames
    check(host_lib, [0, len(bg)], make_meta(bg), max_frames)
    bg.append(0)
    assert run_host(host_lib, [0, len(bg)], make_meta(bg), max_frames)[0] == 2  # SchedError::TooLong


def test_empty_clip(host_lib):
    assert run_host(host_lib, [0, 2, 2, 4], make_meta([0] * 4), 10)[0] == 1  # SchedError::EmptyClip


def test_processed_before(host_lib):
    bg = np.array([1, 1, 0, 0, 1, 0, 0])
    meta = make_meta(bg)
    for n_prev in range(len(bg) + 1):
        assert host_lib.processed_before_host(meta.ctypes.data_as(C.c_void_p), n_prev) == int(np.sum(bg[:n_prev] == 0))


def test_standalone_under_sanitizers(tmp_path):
    """The same source as a program of its own (its main walks the cases above), built with ASan + UBSan."""
    exe = tmp_path / "schedule_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",  # (the runtimes inside the program: nothing to preload)
                           "-DSCHEDULE_HOST_MAIN", *INCLUDES, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
