"""What the GPU tests of the LK kernels share: the process-wide debug hooks as context managers, vh_pyr_lk on one forced route, the bit-for-bit
comparison of its outputs, and the small pair of images whose views have every byte phase and row pitch."""
import contextlib
import ctypes as C

import numpy as np
import pytest


@contextlib.contextmanager
def _hook(name, value, rest):
    from velocity_amd import _lib as L

    fn = getattr(L.load(), name)
    try:
        fn(value)
        yield
    finally:
        fn(rest)


def forced_route(mode):
    """Every LK launch inside the block takes route `mode` (vh_debug_force_generic_lk; 0, restored whatever happens: the library's own routing)."""
    return _hook("vh_debug_force_generic_lk", mode, 0)


def lk3_slots(tpw):
    """The one-wavefront k_lk3 kernels take `tpw` tracks per workgroup inside the block (vh_debug_lk3_tpw; 0: their own choice)."""
    return _hook("vh_debug_lk3_tpw", tpw, 0)


def lk3_one_level(on):
    """on = 0: jobs with max_level = 0 go through the general form of k_lk3 inside the block (vh_debug_lk3_one_level; 1: the single-level form)."""
    return _hook("vh_debug_lk3_one_level", on, 1)


def klt_order(order):
    """The order in which the LK launches walk the tracks inside the block (vh_debug_klt_order; -1: the library's choice)."""
    return _hook("vh_debug_klt_order", order, -1)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_bits(got, exp, ctx):
    """position, status, err (, fbe) of every track as bit patterns; an output that either side does not have is not compared."""
    for name, a, b in zip(("position", "status", "err", "fbe"), got, exp):
        if a is None or b is None:
            continue
        same = (a == b) if a.dtype == bool else (bits(a) == bits(b))
        bad = np.flatnonzero(~same.reshape(len(a), -1).all(1))
        assert not len(bad), (ctx, name, len(bad), bad[:8], a[bad[:8]], b[bad[:8]])


def texture_pair(w, h, seed):
    """Smooth random texture (box-filtered noise, full 8-bit range) and the same texture moved by (+1.5, -1) pixels."""
    rng = np.random.default_rng(seed)
    n = rng.integers(0, 256, (h + 12, w + 12)).astype(np.float64)
    k = np.ones(5) / 5.0
    n = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, n)
    n = np.apply_along_axis(lambda c: np.convolve(c, k, "same"), 0, n)
    n = (n - n.min()) / (n.max() - n.min()) * 255.0
    a = n[6:6 + h, 6:6 + w]
    b = 0.5 * (n[7:7 + h, 4:4 + w] + n[7:7 + h, 5:5 + w])
    return np.rint(a).astype(np.uint8), np.rint(b).astype(np.uint8)


def phase_tracks(w, h):
    """64 points: 40 interior ones whose integer x runs through every residue mod 4 at several sub-pixel offsets, 24 whose 15 x 15 window touches or
    crosses the left, right, top and bottom edge and the four corners."""
    pts = [(20.0 + 1.0 * i + 0.13 * (i % 7), 18.0 + (11 * i) % (h - 36) + 0.29 * (i % 5)) for i in range(40)]
    for k, e in enumerate((0.5, 3.25, 6.75, 7.5)):
        y = 20.0 + 9.5 * k
        pts += [(e, y), (w - 1 - e, y + 3.25), (24.0 + 13.25 * k, e), (30.0 + 11.5 * k, h - 1 - e)]
    pts += [(1.5, 2.25), (w - 2.25, 1.5), (2.75, h - 3.5), (w - 3.5, h - 2.75), (7.0, 7.0), (w - 8.0, h - 8.0), (8.0, h - 8.5), (w - 8.5, 8.0)]
    assert len(pts) == 64
    return np.array(pts, np.float32)


def to_dev(img):
    import torch

    return torch.from_numpy(np.ascontiguousarray(img)).cuda()


def strided_view(img, pitch, phase):
    """`img` as a view into a larger device buffer: rows `pitch` bytes apart, base address = `phase` mod 4."""
    import torch

    h, w = img.shape
    buf = torch.full((h + 4, pitch), 77, dtype=torch.uint8, device="cuda")
    x0 = (phase - 2 * pitch - buf.data_ptr()) & 3
    v = buf[2:2 + h, x0:x0 + w]
    v.copy_(to_dev(img))
    assert v.data_ptr() & 3 == phase and v.stride(0) == pitch and v.stride(1) == 1
    return v


SMALL = dict(win=15, max_level=2, max_count=10, eps=0.03)  # the LK settings of the `small` pair's oracle


@pytest.fixture(scope="module")
def small():
    """-> (I, J, pts, oracle[fbt]): texture_pair(96, 80, 5) and phase_tracks(96, 80) with the CPU oracle's forward and forward-backward result."""
    from oracle import klt_oracle as KO  # (checker only)

    I, J = texture_pair(96, 80, 5)
    pts = phase_tracks(96, 80)
    return I, J, pts, {fbt: KO.lk_fb(I, J, pts, fbt=fbt, **SMALL) for fbt in (None, 1.0)}


def pyr_lk_forced(I, J, pts, fbt, mode, win, max_level, max_count, eps, want_err=True, want_fbe=False):
    """vh_pyr_lk on the forced route `mode`, which the launch must report -> (p2, v, err | None, fbe | None); I, J: device images or views."""
    import torch

    from velocity_amd import _lib as L

    lib = L.load()
    n = len(pts)
    h, w = I.shape
    ws = L.workspace(w, h, n)
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    p2 = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    v = torch.zeros(n, dtype=torch.uint8, device="cuda")
    err = torch.zeros(n, dtype=torch.float32, device="cuda") if want_err else None
    fbe = torch.zeros(n, dtype=torch.float32, device="cuda") if want_fbe else None
    prm = L.lk_params(dict(win=win, max_level=max_level, max_count=max_count, eps=eps))
    routes = (C.c_int * 3)()
    with forced_route(mode):
        L.check(lib.vh_pyr_lk(ws.handle, L.dptr(I), L.dptr(J), w, h, I.stride(0), J.stride(0), L.dptr(p), n, C.byref(prm), C.c_float(-1.0 if fbt is None else fbt),
                              L.dptr(p2), L.dptr(v), L.dptr(err), L.dptr(fbe), L.stream_ptr()), "vh_pyr_lk")
        L.check(lib.vh_profile_lk_routes(ws.handle, routes, None), "vh_profile_lk_routes")
    assert int(routes[0]) == mode, (mode, int(routes[0]))
    return (p2.cpu().numpy(), v.cpu().numpy().astype(bool), None if err is None else err.cpu().numpy(), None if fbe is None else fbe.cpu().numpy())
