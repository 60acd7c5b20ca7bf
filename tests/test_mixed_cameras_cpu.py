"""Streams of different cameras, the parts that need no GPU: the binding of vh_clip_camera against the header's layout, the new entry points among the
declared symbols, and run_queue's size rule (velocity_amd.driver.queue_clip_fits, a pure function like queue_plan)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from velocity_amd import _lib as L
from velocity_amd.driver import queue_clip_fits

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "velocity_hip.h")
CTYPES = {"int": C.c_int, "double": C.c_double}


def _header_struct(name):
    """[(field, ctype)] of `typedef struct name { ... } name;` in the header: scalar and one-dimensional array members of int / double."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), open(HEADER).read(), re.S).group(1)
    fields = []
    for kind, names in re.findall(r"\b(int|double)\s+([^;]+);", body):
        for item in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", item)
            fields.append((m.group(1), CTYPES[kind] * int(m.group(2)) if m.group(2) else CTYPES[kind]))
    return fields


def test_clip_camera_has_the_headers_layout():
    fields = _header_struct("vh_clip_camera")
    assert [f for f, _ in fields] == ["w", "h", "stride", "k_is_float32", "K"]

    class FromHeader(C.Structure):
        _fields_ = fields

    assert C.sizeof(L.ClipCamera) == C.sizeof(FromHeader) == 4 * 4 + 9 * 8
    for name, _ in fields:
        assert getattr(L.ClipCamera, name).offset == getattr(FromHeader, name).offset and getattr(L.ClipCamera, name).size == getattr(FromHeader, name).size, name


def test_clip_camera_from_a_float32_K():
    K = np.float32([[700, 0, 0], [0, 701, 0], [240.5, 135.5, 1]])
    cam = L.clip_camera(480, 270, K)
    assert (cam.w, cam.h, cam.stride, cam.k_is_float32) == (480, 270, 480, 1) and list(cam.K) == [float(v) for v in K.reshape(9)]
    cam = L.clip_camera(414, 233, K.astype(np.float64), stride=416)
    assert (cam.w, cam.h, cam.stride, cam.k_is_float32) == (414, 233, 416, 0)


def test_the_new_entry_points_are_declared_and_bound():
    declared = L.declared_symbols()
    for s in ("vh_session_set_camera", "vh_frame0_init_batch3"):
        assert s in declared and s in L._SIGS, s
    assert L._SIGS["vh_frame0_init_batch3"][1][3] == C.POINTER(L.ClipCamera)
    assert len(L._SIGS["vh_frame0_init_batch3"][1]) == len(L._SIGS["vh_frame0_init_batch2"][1]) - 3  # one camera table for w, h, stride, K_host
    lib = L.load()
    assert lib.vh_version() == 111 and hasattr(lib, "vh_session_set_camera") and hasattr(lib, "vh_frame0_init_batch3")


def test_queue_clip_fits_each_side():
    assert queue_clip_fits(0, (270, 480), (270, 480)) == (270, 480)
    assert queue_clip_fits(3, (233, 414), (270, 480)) == (233, 414)
    assert queue_clip_fits(1, (233, 414, 3), (270, 480)) == (233, 414)  # (a frame's shape may carry more than two entries)
    with pytest.raises(ValueError, match=r"clip 6 has 640 x 480 frames, larger than max_size = 480 x 270"):
        queue_clip_fits(6, (480, 640), (270, 480))
    with pytest.raises(ValueError, match=r"clip 2 has 270 x 480 frames"):  # portrait in a landscape session of the same area: refused, not clipped
        queue_clip_fits(2, (480, 270), (270, 480))
    with pytest.raises(ValueError, match="clip 4"):
        queue_clip_fits(4, (271, 480), (270, 480))
