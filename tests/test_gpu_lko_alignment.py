"""The row loads of the 8- and 4-tracks-per-wavefront kernels (k_lk_o, k_lk_q) at every byte phase.

Their interior paths keep the dwords a lane loaded and fold the byte phase of the address into the v_perm selector of every byte pair
(load_rows_words / pair_selectors in vh_lk.hip), one phase for all the rows a lane loads together.  What can go wrong there depends only on the low
two bits of addresses, so the shapes are the smallest that have every case: images of 96 x 80 (and one of 576 x 480) taken as views into a larger
buffer, so that the base address of level 0 has each phase 0..3 -- a different one for the two images -- and rows 132..135 bytes apart, so that
the phase stays (132) or changes from row to row (133, 134, 135: the further rows of a lane are then dword loads at unaligned addresses).  Three
pyramid levels: level 0 is the caller's view (no border ring), levels 1 and 2 of the small image carry the library's border ring, level 1 of the
large one (288 x 240 > 65536 pixels) does not.  64 tracks whose x positions cover the four phases, with windows that touch and cross every image
edge (border and byte paths next to the interior one in the same wavefront), the forward and the forward-backward pass.

Route 8 (k_lk_o), route 4 (k_lk_q) and the generic k_lk (route 1, plain byte loads) must agree bit for bit in position, status and err, and with
the CPU oracle (which sees the same pixels at every pitch and phase)."""
import ctypes as C

import numpy as np
import pytest

from oracle import klt_oracle as KO  # (checker only)

pytestmark = pytest.mark.gpu

WIN, LEVELS, MAX_COUNT, EPS = 15, 2, 10, 0.03
ROUTES = (8, 4, 1)
PITCHES = (132, 133, 134, 135)


def _texture(w, h, seed):
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


def _tracks(w, h):
    """64 points: 40 interior ones whose integer x runs through every residue mod 4 at several sub-pixel offsets, 24 whose 15 x 15 window touches or
    crosses the left, right, top and bottom edge and the four corners."""
    pts = [(20.0 + 1.0 * i + 0.13 * (i % 7), 18.0 + (11 * i) % (h - 36) + 0.29 * (i % 5)) for i in range(40)]
    for k, e in enumerate((0.5, 3.25, 6.75, 7.5)):
        y = 20.0 + 9.5 * k
        pts += [(e, y), (w - 1 - e, y + 3.25), (24.0 + 13.25 * k, e), (30.0 + 11.5 * k, h - 1 - e)]
    pts += [(1.5, 2.25), (w - 2.25, 1.5), (2.75, h - 3.5), (w - 3.5, h - 2.75), (7.0, 7.0), (w - 8.0, h - 8.0), (8.0, h - 8.5), (w - 8.5, 8.0)]
    assert len(pts) == 64
    return np.array(pts, np.float32)


def _view(img, pitch, phase):
    """`img` as a view into a larger device buffer: rows `pitch` bytes apart, base address = `phase` mod 4."""
    import torch

    h, w = img.shape
    buf = torch.full((h + 4, pitch), 77, dtype=torch.uint8, device="cuda")
    x0 = (phase - 2 * pitch - buf.data_ptr()) & 3
    v = buf[2:2 + h, x0:x0 + w]
    v.copy_(torch.from_numpy(img).cuda())
    assert v.data_ptr() & 3 == phase and v.stride(0) == pitch and v.stride(1) == 1
    return v


def _run(I, J, pts, fbt, mode):
    from velocity_amd import _lib as L
    from velocity_amd.KLT import cv2calcOpticalFlowPyrLK

    lib = L.load()
    try:
        lib.vh_debug_force_generic_lk(mode)
        p2, v, err = cv2calcOpticalFlowPyrLK(I, J, pts, None, fbt=fbt, winSize=(WIN, WIN), maxLevel=LEVELS, criteria=(3, MAX_COUNT, EPS))
        ws = L.workspace(I.shape[1], I.shape[0], len(pts))
        routes = (C.c_int * 3)()
        L.check(lib.vh_profile_lk_routes(ws.handle, routes, None), "vh_profile_lk_routes")
    finally:
        lib.vh_debug_force_generic_lk(0)
    assert int(routes[0]) == mode, (mode, int(routes[0]))
    return np.asarray(p2), np.asarray(v, bool), np.asarray(err).ravel()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_same(got, exp, ctx):
    for name, a, b in zip(("position", "status", "err"), got, exp):
        same = (a == b) if a.dtype == bool else (_bits(a) == _bits(b))
        bad = np.flatnonzero(~same.reshape(len(a), -1).all(1))
        assert not len(bad), (ctx, name, bad[:8], a[bad[:8]], b[bad[:8]])


@pytest.fixture(scope="module")
def small():
    I, J = _texture(96, 80, 5)
    pts = _tracks(96, 80)
    oracle = {fbt: KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS) for fbt in (None, 1.0)}
    return I, J, pts, oracle


@pytest.mark.parametrize("pitch", PITCHES)
def test_every_phase_and_pitch(small, pitch):
    I, J, pts, oracle = small
    for phase in range(4):
        a, b = _view(I, pitch, phase), _view(J, pitch + (phase & 1), (phase + 1 + (pitch & 1)) & 3)
        for fbt in (None, 1.0):
            res = {mode: _run(a, b, pts, fbt, mode) for mode in ROUTES}
            for mode in ROUTES[:2]:
                _assert_same(res[mode], res[1], (pitch, phase, fbt, mode, "generic"))
            for mode in ROUTES:
                _assert_same(res[mode], oracle[fbt], (pitch, phase, fbt, mode, "oracle"))
            assert res[1][1].sum() >= 40, (pitch, phase, fbt, int(res[1][1].sum()))  # the interior tracks are tracked: the comparison is not one of failures


def test_level_without_border_ring():
    """576 x 480: level 1 (288 x 240) is too large for the library's border ring, so a border window there takes the byte loads and an interior one
    the dword loads of a dense level; pitch 579 changes the phase of level 0 from row to row."""
    I, J = _texture(576, 480, 6)
    pts = _tracks(576, 480)
    a, b = _view(I, 579, 3), _view(J, 580, 1)
    for fbt in (None, 1.0):
        res = {mode: _run(a, b, pts, fbt, mode) for mode in ROUTES}
        exp = KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS)
        for mode in ROUTES:
            _assert_same(res[mode], exp, (fbt, mode))
        assert exp[1].sum() >= 40, (fbt, int(exp[1].sum()))
