"""tq_subsample_draw, the stand-alone export of the minibatch subsample (include/tapqir_hip.h): header, binding and library
agree on it, and every bad argument is answered before anything touches a device (no GPU needed)."""

import ctypes
import os
import re

import pytest

from tapqir_amd import _lib
from tapqir_amd.models.engine import CosmosEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_binding_and_library_agree_on_the_export():
    text = open(os.path.join(ROOT, "include", "tapqir_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.findall(r"\bint\s+tq_subsample_draw\s*\(([^)]*)\)", text)
    assert len(decl) == 1
    types = [re.sub(r"\s*\w+$", "", p.strip()) for p in decl[0].split(",")]
    assert types == ["uint64_t", "uint32_t", "int32_t", "int32_t", "int32_t", "int32_t*", "void*"]
    assert "tq_subsample_draw" in _lib.EXPORTS
    fn = _lib.load().tq_subsample_draw
    assert fn.restype is ctypes.c_int
    assert fn.argtypes == [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                           ctypes.c_void_p]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "tq_subsample_draw")
    assert callable(getattr(CosmosEngine, "draw_subsample_device"))


def test_subsample_max_is_the_16_bit_index_field():
    assert _lib.SUBSAMPLE_MAX == 65536


_OUT = (ctypes.c_int32 * 4)()  # (kept alive here) never written: every case below is refused on the host
OUT = ctypes.addressof(_OUT)
BAD_ARGUMENTS = [
    (0, 8, 4, None),       # out == NULL
    (0, 0, 1, OUT),        # n < 1
    (1, -3, 1, OUT),
    (0, 8, 0, OUT),        # take < 1
    (1, 8, -1, OUT),
    (0, 8, 9, OUT),        # take > n
    (1, 65537, 4, OUT),    # n > TQ_SUBSAMPLE_MAX
    (0, 2 ** 31 - 1, 4, OUT),
    (2, 8, 4, OUT),        # axis not 0 or 1
    (-1, 8, 4, OUT),
]


# (ids by hand: the address of _OUT differs from process to process, and a test's id must not)
@pytest.mark.parametrize("axis,n,take,out", BAD_ARGUMENTS,
                         ids=["%d-%d-%d-%s" % (a, n, t, "None" if o is None else "OUT") for a, n, t, o in BAD_ARGUMENTS])
def test_bad_arguments_are_refused_without_a_gpu(axis, n, take, out):
    lib = _lib.load()
    lib.tq_cosmos_step(ctypes.byref(_lib.CosmosArgs()), None)  # (leaves another call's text behind)
    before = lib.tq_last_error()
    assert lib.tq_subsample_draw(7, 1, axis, n, take, out, None) == 1  # TQ_ERR_ARG
    text = lib.tq_last_error()
    assert text and text != before and b"tq_subsample_draw" in text
