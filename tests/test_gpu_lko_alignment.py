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

from lk_support import assert_same_bits as _assert_same
from lk_support import SMALL, forced_route, phase_tracks, small, strided_view, texture_pair  # noqa: F401 (small: a fixture)
from oracle import klt_oracle as KO  # (checker only)

pytestmark = pytest.mark.gpu

WIN, LEVELS, MAX_COUNT, EPS = 15, 2, 10, 0.03
assert dict(win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS) == SMALL  # the `small` fixture's oracle ran with these
ROUTES = (8, 4, 1)
PITCHES = (132, 133, 134, 135)


def _run(I, J, pts, fbt, mode):
    from velocity_amd import _lib as L
    from velocity_amd.KLT import cv2calcOpticalFlowPyrLK

    with forced_route(mode):
        p2, v, err = cv2calcOpticalFlowPyrLK(I, J, pts, None, fbt=fbt, winSize=(WIN, WIN), maxLevel=LEVELS, criteria=(3, MAX_COUNT, EPS))
        ws = L.workspace(I.shape[1], I.shape[0], len(pts))
        routes = (C.c_int * 3)()
        L.check(L.load().vh_profile_lk_routes(ws.handle, routes, None), "vh_profile_lk_routes")
    assert int(routes[0]) == mode, (mode, int(routes[0]))
    return np.asarray(p2), np.asarray(v, bool), np.asarray(err).ravel()


@pytest.mark.parametrize("pitch", PITCHES)
def test_every_phase_and_pitch(small, pitch):
    I, J, pts, oracle = small
    for phase in range(4):
        a, b = strided_view(I, pitch, phase), strided_view(J, pitch + (phase & 1), (phase + 1 + (pitch & 1)) & 3)
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
    I, J = texture_pair(576, 480, 6)
    pts = phase_tracks(576, 480)
    a, b = strided_view(I, 579, 3), strided_view(J, 580, 1)
    for fbt in (None, 1.0):
        res = {mode: _run(a, b, pts, fbt, mode) for mode in ROUTES}
        exp = KO.lk_fb(I, J, pts, fbt=fbt, win=WIN, max_level=LEVELS, max_count=MAX_COUNT, eps=EPS)
        for mode in ROUTES:
            _assert_same(res[mode], exp, (fbt, mode))
        assert exp[1].sum() >= 40, (fbt, int(exp[1].sum()))
