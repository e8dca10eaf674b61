"""The Python side of the C ABI, stated once in cpx._lib: the signature table agrees with include/cpx.h parameter for
parameter, ptr() turns what call sites hold into what ctypes takes and refuses strided memory, call() / status()
marshal by the table and report the status.  No GPU: the checked call runs against a stub library."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from cpx import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_prototypes():
    """{name: [parameter text, ...]} of every cpx_* prototype in include/cpx.h; `(void)` is no parameter."""
    hdr = open(os.path.join(REPO, "include", "cpx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    out = {}
    for m in re.finditer(r"^\s*(?:int|long|void|size_t|const char\*|void\*)\s+(cpx_[a-z_0-9]+)\s*\(", hdr, re.M):
        depth, k = 1, m.end()
        while depth:   # up to the parenthesis that closes the parameter list, across lines
            depth += {"(": 1, ")": -1}.get(hdr[k], 0)
            k += 1
        params = " ".join(hdr[m.end():k - 1].split())
        out[m.group(1)] = [] if params in ("", "void") else [p.strip() for p in params.split(",")]
    return out


PROTOTYPES = header_prototypes()


def is_pointer(ctype):
    return ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer)


def test_table_names_are_the_headers():
    assert len(PROTOTYPES) > 60, "no prototypes found in cpx.h"
    assert set(PROTOTYPES) == set(_lib.SIGNATURES)
    assert _lib.EXPORTS == list(_lib.SIGNATURES)


@pytest.mark.parametrize("name", sorted(_lib.SIGNATURES))
def test_arity_matches_the_header(name):
    assert len(_lib.SIGNATURES[name][1]) == len(PROTOTYPES[name]), PROTOTYPES[name]


@pytest.mark.parametrize("name", ["cpx_track_batch_ex", "cpx_crop_tile", "cpx_graph_create"])
def test_pointer_positions_match_the_header(name):
    declared = [is_pointer(ty) for ty in _lib.SIGNATURES[name][1]]
    assert declared == ["*" in p for p in PROTOTYPES[name]], PROTOTYPES[name]
    assert any(declared) and not all(declared)


def test_load_declares_the_table():
    lib = _lib.load()
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
        assert fn.errcheck is None, name   # callers of the raw functions read the integer status themselves
        assert [k for k, _ in fn.pointers] == [k for k, ty in enumerate(argtypes) if is_pointer(ty)], name


def test_ptr_none_is_null():
    assert _lib.ptr(None) is None
    assert C.c_void_p.from_param(_lib.ptr(None)) is None   # what ctypes passes as NULL


def test_ptr_tensor():
    x = torch.zeros(4)
    got = _lib.ptr(x)
    assert type(got) is C.c_void_p and got.value == x.data_ptr()
    with pytest.raises(ValueError, match="cpx_some_call.*not contiguous"):
        _lib.ptr(torch.zeros(4, 4)[:, 1], "cpx_some_call")


def test_ptr_array():
    a = np.zeros(3, np.int32)
    got = _lib.ptr(a)
    assert type(got) is C.c_void_p and got.value == a.ctypes.data
    with pytest.raises(ValueError, match="cpx_some_call.*not C-contiguous"):
        _lib.ptr(np.zeros((4, 4))[:, 1], "cpx_some_call")


def test_ptr_structure_reaches_the_callee_as_its_address():
    cfg = _lib.Config(160, 120, 1, 45, 20.0, 0.1, 64, 512, 0, 0)
    seen = []

    @C.CFUNCTYPE(C.c_int, C.POINTER(_lib.Config))
    def callee(p):
        seen.append((C.addressof(p.contents), p.contents.width))
        return 0

    assert callee(_lib.ptr(cfg)) == 0
    assert seen == [(C.addressof(cfg), 160)]


def test_ptr_passes_the_rest_through():
    v = C.c_void_p(1234)
    ref = C.byref(C.c_int(3))
    for x in (7, 2.5, b"raw", v, ref):
        assert _lib.ptr(x) is x


class StubLibrary:
    """Stands for the loaded library: cpx_x answers `rc`, and carries its entry of the table as load() gives it to a
    ctypes function."""

    def __init__(self, rc):
        self.calls, self.asked = [], []

        def cpx_x(*args):
            self.calls.append(args)
            return rc

        _lib.declare(cpx_x, C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int32), C.c_double, C.c_void_p])
        self.cpx_x = cpx_x

    def cpx_last_error(self, handle):
        self.asked.append(handle)
        return b"boom"


def stub_arguments():
    return C.c_void_p(99), torch.zeros(4), 5, np.arange(3, dtype=np.int32), 0.5, None


def check_marshalled(stub, args):
    (h, x, n, offs, lr, nothing), = stub.calls
    assert h is args[0]
    assert type(x) is C.c_void_p and x.value == args[1].data_ptr()
    assert type(n) is int and n == 5
    assert isinstance(offs, C.POINTER(C.c_int32)) and C.addressof(offs.contents) == args[3].ctypes.data and offs[2] == 2
    assert type(lr) is float and lr == 0.5
    assert nothing is None


def test_call_raises_the_status_with_the_handles_message():
    stub, args = StubLibrary(-2), stub_arguments()
    with pytest.raises(_lib.CpxError) as e:
        _lib.call(stub, args[0], "cpx_x", *args)
    assert e.value.code == -2 and "boom" in str(e.value) and "CPX_ERR_UNSUPPORTED (-2)" in str(e.value)
    assert stub.asked == [args[0]]
    check_marshalled(stub, args)


def test_status_returns_the_status():
    stub, args = StubLibrary(-2), stub_arguments()
    assert _lib.status(stub, "cpx_x", *args) == -2
    assert stub.asked == []
    check_marshalled(stub, args)


def test_call_returns_on_ok():
    stub, args = StubLibrary(0), stub_arguments()
    assert _lib.call(stub, args[0], "cpx_x", *args) is None
    assert stub.asked == []
    check_marshalled(stub, args)


def test_call_refuses_strided_memory_and_a_wrong_count():
    stub, args = StubLibrary(0), list(stub_arguments())
    with pytest.raises(TypeError, match="cpx_x takes 6"):
        _lib.call(stub, args[0], "cpx_x", *args[:-1])
    args[1] = torch.zeros(4, 4)[:, 1]
    with pytest.raises(ValueError, match="cpx_x"):
        _lib.call(stub, args[0], "cpx_x", *args)
    assert stub.calls == []
    stub.cpx_y = lambda *a: 0   # a function nobody declared: refused by name, not by a missing attribute
    with pytest.raises(TypeError, match="cpx_y has no declared prototype"):
        _lib.status(stub, "cpx_y", *args)
