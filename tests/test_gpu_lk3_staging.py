"""k_lk3's region staging and its first Newton iteration against the CPU oracle, bit for bit.

(a) stage_region: four dwords per lane (one 16-byte load and the dword behind it), 4 / 2 lanes per region row.  What decides its addresses and byte phases is
    the row pitch, the byte phase of the image's base pointer and where the staged rectangle lies against the limits of its `fast` predicate -- so the same
    tracks run on row pitches that are a multiple of 16, of 4 only, and odd, from a base pointer at each byte phase, with the template patch and the
    search region exactly at and one pixel past each of the four limits (rx == 0, rx + WIDTH + 4 == w, ry == 0, ry + ROWS == h), through every
    instantiation of the kernel; a second frame pair moves the tracks further than the search margin, so that the region is staged again (`restage`).
(b) The first iteration of a top level takes its origin and weights from the template set-up (lk_iter_at_template_origin): one- and three-level jobs, integer
    and fractional start points, max_count = 1 (nothing but that iteration runs) and the default, with and without the backward pass.
(c) A job with max_level = 0 takes the single-level form of the kernel (lk_track<ONE_LEVEL>); vh_debug_lk3_one_level(0) sends it through the general form,
    whose level loop then runs once.  (a) and (b) run their one-level jobs through both forms; every result must be the oracle's, hence the same."""
import functools

import numpy as np
import pytest

from oracle import klt_oracle as KO  # (checker only)
from lk_support import forced_route, lk3_one_level, lk3_slots
from test_gpu_klt import _lib

# window -> modes of forced_route -> search margin M, staged bytes per patch row / per region row (LK3::PI_PITCH, LK3::PJ_WIDTH)
GEOM = {51: dict(M=4, patch_w=56, region_w=64, modes=(5, 6, 7)), 15: dict(M=6, patch_w=20, region_w=32, modes=(3,))}
W, H = 130, 100
PITCHES = (144, 132, 131)  # a multiple of 16, of 4 only, odd
FBT = 0.3


def _smooth_noise(h, w, seed, box, passes):
    rng = np.random.default_rng(seed)
    a = rng.random((h, w))
    k = np.ones(box) / box
    for _ in range(passes):
        a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, a)
        a = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, a)
    return 255.0 * (a - a.min()) / (a.max() - a.min())


def _sample(big, x, y):
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    ax, ay = x - x0, y - y0
    return (1 - ay) * ((1 - ax) * big[y0, x0] + ax * big[y0, x0 + 1]) + ay * ((1 - ax) * big[y0 + 1, x0] + ax * big[y0 + 1, x0 + 1])


@functools.lru_cache(maxsize=None)
def _pair(w, h, seed, box, passes, dx, dy):
    """A seeded frame pair of smoothed noise, the second frame displaced by (dx, dy) pixels."""
    pad = 16
    big = _smooth_noise(h + 2 * pad, w + 2 * pad, seed, box, passes)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f0 = np.rint(_sample(big, xx + pad, yy + pad)).astype(np.uint8)
    f1 = np.rint(_sample(big, xx + pad - dx, yy + pad - dy)).astype(np.uint8)
    f0.setflags(write=False)
    f1.setflags(write=False)
    return f0, f1


def _limit_tracks(win):
    """Start points whose template patch (origin (ipx - 1, ipy - 1)) or whose search region (origin (ipx - M, ipy - M)) lies exactly at, and one pixel past,
    each limit of stage_region's `fast` predicate, the other coordinate in the middle of the frame; then two plain interior tracks."""
    g = GEOM[win]
    half = (win - 1) / 2.0
    mid_x, mid_y = (W - win) // 2, (H - win) // 2
    pts = []
    for off, width, rows in ((1, g["patch_w"], win + 3), (g["M"], g["region_w"], win + 1 + 2 * g["M"])):
        for ipx in (off, off - 1, W - width - 4 + off, W - width - 4 + off + 1):  # rx == 0, rx == -1, rx + WIDTH + 4 == w, == w + 1
            pts.append((ipx + half + 0.3, mid_y + half + 0.6))
        for ipy in (off, off - 1, H - rows + off, H - rows + off + 1):  # ry == 0, ry == -1, ry + ROWS == h, == h + 1
            pts.append((mid_x + half + 0.7, ipy + half + 0.2))
    pts += [(mid_x + half, mid_y + half), (mid_x + half + 3.25, mid_y + half - 2.5)]
    return np.array(pts, np.float32)


def _origins(pts, win):
    return np.floor(pts.astype(np.float32) - np.float32((win - 1) * 0.5)).astype(int)


# (a): two frame pairs per window -- "near" moves by less than the search margin, "far" by more (a smoother texture, so that the iterations follow it)
STAGING = {
    (51, "near"): dict(seed=11, box=5, passes=2, dx=1.3, dy=-0.7, lk=dict(win=51, max_level=0, max_count=30, eps=0.001)),
    (51, "far"): dict(seed=12, box=9, passes=3, dx=6.4, dy=-5.3, lk=dict(win=51, max_level=0, max_count=30, eps=0.001)),
    (15, "near"): dict(seed=13, box=5, passes=2, dx=1.3, dy=-0.7, lk=dict(win=15, max_level=0, max_count=10, eps=0.1)),
    (15, "far"): dict(seed=14, box=11, passes=3, dx=8.6, dy=-7.4, lk=dict(win=15, max_level=0, max_count=30, eps=0.01)),
}


@functools.lru_cache(maxsize=None)
def _staging_case(win, motion):
    """(f0, f1, pts, lk, oracle (p, v, err, fbe)): computed once, shared, never written to."""
    sc = STAGING[(win, motion)]
    f0, f1 = _pair(W, H, sc["seed"], sc["box"], sc["passes"], sc["dx"], sc["dy"])
    pts = _limit_tracks(win)
    ref = KO.lk_fb(f0, f1, pts, fbt=FBT, return_fbe=True, **sc["lk"])
    for a in ref:
        a.setflags(write=False)
    return f0, f1, pts, sc["lk"], ref


@pytest.mark.parametrize("win", sorted(GEOM))
def test_the_tracks_stand_at_the_limits_and_the_far_pair_leaves_the_region(win):
    """CPU only: the start points put the staged rectangles where the docstring says, and in the "far" pair the oracle moves live tracks by more than the
    search margin + 1 in x or y, which no iteration can reach without the region being staged again."""
    g = GEOM[win]
    pts = _limit_tracks(win)
    ip = _origins(pts, win)
    for off, width, rows in ((1, g["patch_w"], win + 3), (g["M"], g["region_w"], win + 1 + 2 * g["M"])):
        rx, ry = ip[:, 0] - off, ip[:, 1] - off
        for want in (0, -1, W - width - 4, W - width - 3):
            assert (rx == want).any(), (win, off, want, rx)
        for want in (0, -1, H - rows, H - rows + 1):
            assert (ry == want).any(), (win, off, want, ry)
    for motion in ("near", "far"):
        f0, f1, pts, lk, (p, v, err, fbe) = _staging_case(win, motion)
        fwd, alive, _ = KO.pyr_lk(f0, f1, pts, **lk)
        moved = np.abs(fwd - pts).max(axis=1)
        assert alive.sum() >= 8, (win, motion, alive)
        if motion == "far":
            assert (moved[alive] > g["M"] + 1).sum() >= 4, (win, moved, alive)
        else:
            assert (moved[alive] < g["M"]).all() and v.any(), (win, moved, v)


def _pitched(torch, img, pitch, phase):
    """`img` on the device with rows `pitch` bytes apart and the first pixel `phase` bytes behind a 256-byte boundary; (the buffer -- keep it alive --, pointer)."""
    h, w = img.shape
    buf = torch.full((pitch * h + 260,), 0xA5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    buf[phase:phase + pitch * h].view(h, pitch)[:, :w] = torch.from_numpy(np.array(img)).cuda()
    return buf, buf.data_ptr() + phase


def _run(L, C, torch, ws, pa, pb, w, h, sa, sb, pts, lk, fbt, want_err=True):
    n = len(pts)
    p = torch.from_numpy(np.ascontiguousarray(pts, np.float32)).cuda()
    p2 = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    v = torch.zeros(n, dtype=torch.uint8, device="cuda")
    err = torch.zeros(n, dtype=torch.float32, device="cuda") if want_err else None
    fbe = torch.zeros(n, dtype=torch.float32, device="cuda") if fbt is not None else None
    prm = L.lk_params(lk)
    L.check(ws.lib.vh_pyr_lk(ws.handle, C.c_void_p(pa), C.c_void_p(pb), w, h, sa, sb, L.dptr(p), n, C.byref(prm), C.c_float(-1.0 if fbt is None else fbt),
                             L.dptr(p2), L.dptr(v), L.dptr(err), L.dptr(fbe), L.stream_ptr()), "vh_pyr_lk")
    routes = (C.c_int * 3)()
    L.check(ws.lib.vh_profile_lk_routes(ws.handle, routes, None), "vh_profile_lk_routes")
    return (p2.cpu().numpy(), v.cpu().numpy().astype(bool), None if err is None else err.cpu().numpy(), None if fbe is None else fbe.cpu().numpy(), int(routes[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode, win", [(m, win) for win in sorted(GEOM) for m in GEOM[win]["modes"]])
def test_staging_gives_the_oracles_bits_at_every_pitch_phase_and_limit(mode, win):
    L, C, torch = _lib()
    lib = L.load()
    ws = L.workspace(W, H, 32)
    with forced_route(mode), lk3_slots(0), lk3_one_level(1):  # (the two inner hooks are set per case below and restored here)
        for motion in ("near", "far"):
            f0, f1, pts, lk, (ep, ev, eerr, efbe) = _staging_case(win, motion)
            for pitch in PITCHES:
                for phase in range(4):
                    # the two images take different phases, and the second one another pitch class where the first is the odd one
                    ka, pa = _pitched(torch, f0, pitch, phase)
                    kb, pb = _pitched(torch, f1, pitch + (phase & 1), (phase + 1) & 3)
                    # (c): the single-level form at every combination, the general form with one level once per pitch
                    for tpw, one_level in (((1, 1), (4, 1)) if mode in (3, 5) else ((0, 1),)) + (((4 if mode in (3, 5) else 0, 0),) if phase == 1 else ()):
                        lib.vh_debug_lk3_tpw(tpw)
                        lib.vh_debug_lk3_one_level(one_level)
                        p2, v, err, fbe, route = _run(L, C, torch, ws, pa, pb, W, H, pitch, pitch + (phase & 1), pts, lk, FBT)
                        ctx = (mode, win, motion, pitch, phase, tpw, one_level)
                        assert route == mode, (ctx, route)
                        assert np.array_equal(v, ev), (ctx, v, ev)
                        assert np.array_equal(p2, ep), (ctx, p2, ep)
                        assert np.array_equal(err, eerr), (ctx, err, eerr)
                        assert np.array_equal(fbe, efbe), (ctx, fbe, efbe)
                    del ka, kb


# (b): 224 x 216 is the smallest frame whose third pyramid level (56 x 54) still holds a 51 x 51 window
REUSE = {51: dict(w=224, h=216, seed=21, modes=(5, 6, 7), count=30, eps=0.001), 15: dict(w=W, h=H, seed=22, modes=(3,), count=10, eps=0.1)}


def _reuse_tracks(win, w, h):
    """Integer and fractional start points in the interior, one whose window touches the border (border set-up) and one outside the frame."""
    half = (win - 1) / 2.0
    cx, cy = w // 2, h // 2
    return np.array([(cx, cy), (cx + 9, cy - 6), (cx - 12.0, cy + 7.0), (cx + 0.25, cy + 0.5), (cx - 7.7, cy + 4.3), (cx + 11.5, cy - 8.125),
                     (half - 3.0, cy), (cx + 0.5, h - half + 2.25), (-2.0 * win, cy)], np.float32)


@functools.lru_cache(maxsize=None)
def _reuse_case(win, max_level, max_count, fb):
    cf = REUSE[win]
    f0, f1 = _pair(cf["w"], cf["h"], cf["seed"], 5, 2, 1.6, -1.1)
    pts = _reuse_tracks(win, cf["w"], cf["h"])
    lk = dict(win=win, max_level=max_level, max_count=cf["count"] if max_count is None else max_count, eps=cf["eps"])
    if fb:
        ref = KO.lk_fb(f0, f1, pts, fbt=FBT, return_fbe=True, **lk)
    else:
        ref = KO.lk_fb(f0, f1, pts, fbt=None, **lk) + (None,)
    for a in ref:
        if a is not None:
            a.setflags(write=False)
    return f0, f1, pts, lk, ref


@pytest.mark.gpu
@pytest.mark.parametrize("mode, win", [(m, win) for win in sorted(REUSE) for m in REUSE[win]["modes"]])
def test_first_iteration_on_the_template_origin_gives_the_oracles_bits(mode, win):
    L, C, torch = _lib()
    lib = L.load()
    cf = REUSE[win]
    ws = L.workspace(cf["w"], cf["h"], 32)
    with forced_route(mode), lk3_one_level(1):  # (set per case below, restored here)
        for max_level in (0, 2):
            for max_count in (1, None):
                for fb in (False, True):
                    f0, f1, pts, lk, (ep, ev, eerr, efbe) = _reuse_case(win, max_level, max_count, fb)
                    a, b = torch.from_numpy(np.array(f0)).cuda(), torch.from_numpy(np.array(f1)).cuda()
                    for one_level in ((1, 0) if max_level == 0 else (1,)):  # (c): the hook matters for one-level jobs only
                        lib.vh_debug_lk3_one_level(one_level)
                        p2, v, err, fbe, route = _run(L, C, torch, ws, a.data_ptr(), b.data_ptr(), cf["w"], cf["h"], cf["w"], cf["w"], pts, lk, FBT if fb else None)
                        ctx = (mode, win, max_level, max_count, fb, one_level)
                        assert route == mode, (ctx, route)
                        assert np.array_equal(v, ev), (ctx, v, ev)
                        assert np.array_equal(p2, ep), (ctx, p2, ep)
                        assert np.array_equal(err, eerr), (ctx, err, eerr)
                        if fb:
                            assert np.array_equal(fbe, efbe), (ctx, fbe, efbe)


def test_the_reuse_scenes_have_live_tracks_and_the_levels_asked_for():
    """CPU only: with max_count = 1 and with the default the oracle keeps interior tracks alive (what the GPU test compares is not a column of dead tracks),
    the two iteration caps give different points (the cap is felt), and the three-level frames hold three levels."""
    for win, cf in REUSE.items():
        assert min((cf["w"] + 3) // 4, (cf["h"] + 3) // 4) > win, (win, cf)  # the size of pyramid level 2
        for max_level in (0, 2):
            one = _reuse_case(win, max_level, 1, False)[4]
            full = _reuse_case(win, max_level, None, False)[4]
            assert one[1][:6].all() and full[1][:6].all(), (win, max_level, one[1], full[1])
            assert not one[1][-1] and not full[1][-1]
            assert not np.array_equal(one[0][:6], full[0][:6]), (win, max_level)
