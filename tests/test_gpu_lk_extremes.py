"""Every Lucas-Kanade kernel at worst-case contrast and at the window sizes no other test uses, bit for bit against the CPU oracle (and, for the
single-level forward solve, against the exact-integer model of tests/lk_ref.py directly).

The kernels keep int32 per-lane partial sums, reduce them as 16-bit halves and build bilinear samples with 24-bit multiply-adds, each on the argument
that 8-bit images cannot produce larger operands (the bounds table in DESIGN.md).  The binary scenes of lk_ref come within 4-15 % of the largest Ix.Ix
window sum and reach about half of the largest diff.Ix sum -- the most a binary pair can -- which tests/test_lk_ref_cpu.py asserts."""
import ctypes as C

import numpy as np
import pytest

import lk_ref as R
from lk_support import bits as _bits
from lk_support import forced_route, lk3_slots
from oracle import klt_oracle as KO  # (checker only)
from velocity_amd import synth

pytestmark = pytest.mark.gpu

WINDOWS = (3, 8, 15, 16, 21, 51, 63, 64, 65, 107)  # 63: the last window of the strip kernel (16 strips per lane); 107: dynamic LDS above 64 KiB
SETTINGS = [(fbt, lvl, mc, eps) for fbt in (None, 1.0) for lvl in (0, 2) for mc, eps in R.CRITERIA]
SWEEP_ODD = (3, 5, 7, 9, 13, 17, 25, 33, 47, 49, 53, 59, 61, 63, 65, 71, 107)
SWEEP_EVEN = (4, 8, 16, 20, 64)


def _routes(win):
    """(forced_route mode, lk3_slots count, the route the launch must report | None) of every kernel that solves this window.
    The slot count only exists in the one-wavefront LDS-staged kernel: the default route and route 5 run with 1 and 4 slots per workgroup."""
    if win == 15:
        return [(0, 0, None), (1, 0, 1), (2, 0, 2), (3, 0, 3), (4, 0, 4), (8, 0, 8)]
    if win == 51:  # (default routing: one wavefront per track from 640 tracks in flight -- the four track sets together are 808 -- so the slots apply)
        return [(0, 1, 5), (0, 4, 5), (1, 0, 1), (2, 0, 2), (5, 1, 5), (5, 4, 5), (6, 0, 6), (7, 0, 7)]
    if win <= 63:
        return [(0, 0, 2), (1, 0, 1), (2, 0, 2)]
    return [(0, 0, 1), (1, 0, 1)]


def _run(I, J, pts, win, max_level, max_count, eps, fbt, mode, tpw):
    """(p2, v, err, route) of cv2calcOpticalFlowPyrLK on one forced route; both hooks are process-wide and reset whatever happens.  The slot count the
    launch reports is checked here."""
    from velocity_amd import _lib as L
    from velocity_amd.KLT import cv2calcOpticalFlowPyrLK

    lib = L.load()
    with forced_route(mode), lk3_slots(tpw):
        p2, v, err = cv2calcOpticalFlowPyrLK(I, J, pts, None, fbt=fbt, winSize=(win, win), maxLevel=max_level, criteria=(3, max_count, eps))
        ws = L.workspace(I.shape[1], I.shape[0], len(pts))
        routes, slots = (C.c_int * 3)(), (C.c_int * 3)()
        L.check(lib.vh_profile_lk_routes(ws.handle, routes, None), "vh_profile_lk_routes")
        L.check(lib.vh_profile_lk_tpw(ws.handle, slots), "vh_profile_lk_tpw")
    # the launch slots per workgroup the launch reports: the hook's value in the one-wavefront LDS-staged kernels (routes 3 and 5; 1 when the hook is
    # off, far below the loads at which they take more on their own), 1 in every other kernel
    assert int(slots[0]) == ((tpw or 1) if int(routes[0]) in (3, 5) else 1), (win, mode, tpw, int(routes[0]), int(slots[0]))
    return p2, v, err.ravel(), int(routes[0])


def _assert_same(got, exp, ctx):
    """status, position and err of every track, as bit patterns."""
    p, v, e = got
    ep, ev, ee = exp
    bad = np.flatnonzero(np.asarray(v, bool) != np.asarray(ev, bool))
    assert not len(bad), (ctx, "status", bad[:8])
    bad = np.flatnonzero((_bits(p) != _bits(ep)).any(1))
    assert not len(bad), (ctx, "position", bad[:8], p[bad[:8]], ep[bad[:8]])
    bad = np.flatnonzero(_bits(e) != _bits(ee))
    assert not len(bad), (ctx, "err", bad[:8], e[bad[:8]], ee[bad[:8]])


@pytest.mark.parametrize("scene", sorted(R.SCENES))
@pytest.mark.parametrize("win", WINDOWS)
def test_worst_case_content_on_every_route(win, scene):
    """The four track sets of lk_ref in one launch (tracks are independent), forward and forward-backward, one and three pyramid levels (the upper levels
    of the 2-px checkerboard are flat gray: the min-eigenvalue exit runs above level 0 and status survives), the three criteria, every kernel."""
    I, J = (np.array(a) for a in R.SCENES[scene]())  # (writable copies: torch refuses to wrap read-only arrays quietly)
    sets = [R.tracks(win, o) for o in R.OFFSETS]
    pts = np.concatenate(sets)
    ends = np.cumsum([len(s) for s in sets])
    for fbt, lvl, mc, eps in SETTINGS:
        exp = KO.lk_fb(I, J, pts, fbt=fbt, win=win, max_level=lvl, max_count=mc, eps=eps)
        for mode, tpw, route in _routes(win):
            p, v, e, took = _run(I, J, pts, win, lvl, mc, eps, fbt, mode, tpw)
            ctx = (scene, win, fbt, lvl, mc, eps, mode, tpw)
            assert route is None or took == route, (ctx, took)
            _assert_same((p, v, e), exp, ctx)
            if lvl == 0 and fbt is None:  # the model directly
                for o, lo, hi in zip(R.OFFSETS, ends - [len(s) for s in sets], ends):
                    _assert_same((p[lo:hi], v[lo:hi], e[lo:hi]), R.model(scene, win, o, mc, eps)[:3], ctx + (o, "model"))


def _sweep_scenes():
    m = synth.AffineMotion(R.W, R.H, s=1.003, theta_deg=0.3, tx=1.7, ty=-1.1)
    natural = tuple(synth.render_frame(R.W, R.H, m, k, seed=63).numpy() for k in (0, 1))
    return tuple((name, tuple(np.array(a) for a in pair)) for name, pair in (("bars16", R.bars(16)), ("checker3", R.checker(3)), ("render_frame", natural)))


@pytest.mark.parametrize("win", SWEEP_ODD + SWEEP_EVEN)
def test_window_sweep(win):
    """Windows nothing else runs -- the strip kernel from 3 to its limit of 63, the per-sample kernel above, even windows, the first window whose per-sample
    LDS needs the opt-in above 64 KiB (107) -- on worst-case bars, a checkerboard and a rendered pair, with the forward-backward gate."""
    pts = np.array(R.tracks(win, "rand"))
    for name, (I, J) in _sweep_scenes():
        for lvl in (0, 2):
            exp = KO.lk_fb(I, J, pts, fbt=1.0, win=win, max_level=lvl, max_count=10, eps=0.03)
            for mode in (0, 1, 2):
                p, v, e, took = _run(I, J, pts, win, lvl, 10, 0.03, 1.0, mode, 0)
                assert took == (1 if win > 63 or mode == 1 else 2 if win not in (15, 51) or mode == 2 else took), (name, win, lvl, mode, took)
                _assert_same((p, v, e), exp, (name, win, lvl, mode))


def test_window_too_large_for_lds_is_refused_before_anything_runs():
    """win = 166 is the first window whose per-sample LDS exceeds a workgroup's 160 KiB (ceil(166^2 / 64) * 384 = 165 504 > 163 840; 165 needs 163 584):
    at 166 and 167 vh_pyr_lk returns non-zero, names the window and the limit, leaves the outputs alone, and the context serves the next call."""
    from velocity_amd import _lib as L

    torch = L.torch_cuda()
    lib = L.load()
    I, J = R.bars(16)
    pts = R.tracks(15, "rand")
    n = len(pts)
    a, b = torch.from_numpy(np.array(I)).cuda(), torch.from_numpy(np.array(J)).cuda()
    p = torch.from_numpy(np.array(pts)).cuda()
    ws = L.Workspace(1, R.W, R.H, n)

    def call(win):
        p2 = torch.full((n, 2), -7.0, dtype=torch.float32, device="cuda")
        v = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
        err = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
        prm = L.lk_params(dict(win=win, max_level=0, max_count=10, eps=0.03))
        rc = lib.vh_pyr_lk(ws.handle, L.dptr(a), L.dptr(b), R.W, R.H, R.W, R.W, L.dptr(p), n, C.byref(prm), C.c_float(-1.0), L.dptr(p2), L.dptr(v), L.dptr(err),
                           None, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, p2.cpu().numpy(), v.cpu().numpy(), err.cpu().numpy()

    for win in (167, 166):
        rc, p2, v, err = call(win)
        assert rc != 0, win
        msg = lib.vh_last_error().decode()
        assert str(win) in msg and "165" in msg, msg
        assert (p2 == -7.0).all() and (v == 9).all() and (err == -7.0).all(), win
    rc, p2, v, err = call(15)
    assert rc == 0, lib.vh_last_error().decode()
    _assert_same((p2, v, err), KO.pyr_lk(I, J, pts, win=15, max_level=0, max_count=10, eps=0.03), 15)
