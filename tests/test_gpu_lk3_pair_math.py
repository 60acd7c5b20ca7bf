"""The one-wavefront k_lk3 kernels (<51, 1, 4>, route 5, and <15, 1, 6>, route 3) run a track's x and y arithmetic in two lanes of one register (the pair
form of velocity_amd/csrc/vh_lk_shared.hpp).  A scene that treats x and y alike cannot tell a pair whose halves were exchanged, or a stop rule that looked
at one half only, from a correct one; these scenes do not treat them alike.  Every case is p, status, err and fbe of EVERY track, forward plus backward pass,
bit for bit against the CPU oracle (oracle/klt_oracle); the bars scenes also against the exact-integer model of tests/lk_ref.py.

* anisotropic texture: strong bars along one axis over a faint isotropic texture (the system stays solvable, one axis carries ~100 x the gradient energy of
  the other; these do the work on the Newton update), a mix, and bars ALONE, vertical and horizontal: those two kill every track at the determinant gate, so
  they test the set-up only -- the converted sums and the gate with the large sum on either side of the pair (s11 against s22); shifted by (0.3, 0), (0, 0.3), (0.49, -0.51) and by whole pixels -- the eps test and the
  +-0.01 rule then see a large step on one axis and a small one on the other, and on different iterations;
* max_count 1, 2, 3, 30 x eps 0.1, 0.001, 0 (with eps = 0 only the oscillation rule and the cap end a level);
* tracks whose window origin is negative on one axis only, and tracks on both sides of the leave-the-level rule at one edge only (floor of negative values,
  lk_outside, status 0 from the final origin); under a 3 px shift one of them per axis walks out through the left / the top edge DURING the iterations
  (alive after one Newton step, dead after two: with three or thirty steps the rule inside the loop is what ends it);
* a 6 px shift: the search region is staged again and the integer origin changes between iterations;
* bars16 / bars16_neg of tests/lk_ref.py, whose first window sums reach +-85 x 2^31: both signs through the conversion of the summed 16-bit halves."""
import functools

import numpy as np
import pytest

import lk_ref as R
from lk_support import bits as _bits
from lk_support import forced_route, lk3_slots
from oracle import klt_oracle as KO  # (checker only)
from test_gpu_klt import _lib, _pyr_lk_raw
from test_gpu_lk3_track_loop import _bilinear

W, H = R.W, R.H  # 192 x 160
FBT = 0.5
ROUTES = {51: 5, 15: 3}  # window -> the forced_route mode of its one-wavefront k_lk3 kernel
LEVELS = (0, 2)  # max_level: 1 and 3 pyramid levels
CRITERIA = tuple((mc, eps) for mc in (1, 2, 3, 30) for eps in (0.1, 0.001, 0.0))
TEXTURES = ("vbars", "hbars", "mix", "vbars_only", "hbars_only")
LEAVING = (("mix", (-3.0, 0.0), 44), ("mix", (0.0, -3.0), 45))  # (texture, shift, the track that leaves through the left / the top edge inside the loop)
SHIFTS = ((0.3, 0.0), (0.0, 0.3), (0.49, -0.51), (2.0, -1.0), (0.0, 3.0))
PAD = 16


@functools.lru_cache(maxsize=None)
def _noise():
    rng = np.random.default_rng(5115)
    big = rng.random((H + 2 * PAD, W + 2 * PAD))
    k = np.ones(5) / 5.0
    for _ in range(2):
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 0, big)
        big = np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), 1, big)
    return (big - big.min()) / (big.max() - big.min()) - 0.5  # [-0.5, 0.5]


def _render(texture, dx, dy):
    """The texture as a function of the plane, sampled at (x - dx, y - dy) and rounded to 8 bits."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    x, y = xx - dx, yy - dy
    ax, ay, an = {"vbars": (90.0, 0.0, 16.0), "hbars": (0.0, 90.0, 16.0), "mix": (55.0, 55.0, 16.0), "vbars_only": (100.0, 0.0, 0.0), "hbars_only": (0.0, 100.0, 0.0), "smooth": (0.0, 0.0, 250.0)}[texture]
    f = 128.0 + ax * np.sin(2.0 * np.pi * x / 9.3) + ay * np.sin(2.0 * np.pi * y / 11.7 + 0.4) + an * _bilinear(_noise(), x + PAD, y + PAD)
    return np.ascontiguousarray(np.rint(np.clip(f, 0.0, 255.0)).astype(np.uint8))


@functools.lru_cache(maxsize=None)
def _pair(texture, shift):
    if texture in R.SCENES:
        return tuple(np.array(a) for a in R.SCENES[texture]())  # (writable copies: torch refuses to wrap read-only arrays quietly)
    return _render(texture, 0.0, 0.0), _render(texture, *shift)


@functools.lru_cache(maxsize=None)
def _tracks(win):
    """At most 64 tracks: a 6 x 4 grid inside the frame at seeded fractions; windows whose origin is negative, or whose far side is past the frame, on ONE axis
    (the other coordinate in the middle of the frame); and start points on both sides of the rule that drops a track whose window origin lies further than
    `win` outside the level, again at one edge at a time."""
    rng = np.random.default_rng(5100 + win)
    half = (win - 1) / 2.0
    lo = half + 2.0
    gx, gy = np.meshgrid(np.linspace(lo, W - 2.0 - lo, 6), np.linspace(lo, H - 2.0 - lo, 4))
    grid = np.stack([gx.ravel(), gy.ravel()], 1) + rng.random((24, 2))
    cx, cy = W / 2.0 + 0.37, H / 2.0 + 0.61
    one_axis = [(half - 3.7, cy), (cx, half - 2.2), (W - 1 - half + 3.3, cy), (cx, H - 1 - half + 2.6), (0.4, cy), (cx, 0.7), (W - 1.3, cy), (cx, H - 1.6)]
    edge = []
    for d in (-1.5, -0.3, 0.3, 1.5):  # the origin p - half against -win (left / top) and against w, h (right / bottom): both sides of each
        edge += [(-win + half + d, cy), (cx, -win + half + d), (W + half + d, cy), (cx, H + half + d)]
    pts = np.array(list(grid) + one_axis + edge, np.float32)
    assert len(pts) <= 64
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def _oracle(texture, shift, win, max_level, max_count, eps):
    """(p, status, err, fbe) of every track: computed once, shared, never written to."""
    I, J = _pair(texture, shift)
    out = KO.lk_fb(I, J, np.array(_tracks(win)), fbt=FBT, return_fbe=True, win=win, max_level=max_level, max_count=max_count, eps=eps)
    for a in out:
        a.setflags(write=False)
    return out


def _check_pair(texture, shift, criteria=CRITERIA, model=None):
    """One frame pair, uploaded once: both windows on their one-wavefront routes x 1 and 3 levels x the criteria."""
    L, C, torch = _lib()
    I, J = _pair(texture, shift)
    a, b = torch.from_numpy(I).cuda(), torch.from_numpy(J).cuda()
    for win, mode in ROUTES.items():
        pts = np.array(_tracks(win))
        ws = L.workspace(W, H, len(pts))
        with forced_route(mode), lk3_slots(1):
            for max_level in LEVELS:
                for max_count, eps in criteria:
                    lk = dict(win=win, max_level=max_level, max_count=max_count, eps=eps)
                    ep, ev, eerr, efbe = _oracle(texture, shift, win, max_level, max_count, eps)
                    p, v, err, fbe, route, used = _pyr_lk_raw(ws, a, b, W, H, pts, lk, FBT, True, True)
                    ctx = (texture, shift, win, max_level, max_count, eps)
                    assert route == mode and used == 1, (ctx, route, used)
                    bad = np.flatnonzero(np.asarray(v, bool) != np.asarray(ev, bool))
                    assert not len(bad), (ctx, "status", bad, pts[bad])
                    bad = np.flatnonzero((_bits(p) != _bits(ep)).any(1))
                    assert not len(bad), (ctx, "p", bad, p[bad], ep[bad])
                    bad = np.flatnonzero(_bits(err) != _bits(eerr))
                    assert not len(bad), (ctx, "err", bad, err[bad], eerr[bad])
                    bad = np.flatnonzero(_bits(fbe) != _bits(efbe))
                    assert not len(bad), (ctx, "fbe", bad, fbe[bad], efbe[bad])
                    if model is not None and max_level == 0:  # the forward pass of the exact-integer model: position wherever the oracle's gate let it stand
                        mp, ms, _, _ = model(win, max_count, eps)
                        live = np.asarray(ev, bool)
                        assert (_bits(p[live]) == _bits(mp[live])).all() and ms[live].all(), (ctx, "model")


def test_the_scenes_do_what_they_are_for():
    """CPU only (the oracle alone): the anisotropic scenes are solvable and anisotropic, bars alone are not solvable, the 6 px scene moves live tracks of the
    51 x 51 window out of the +-4 px the staged region holds, the edge tracks fall on both sides of the status rule, and the criteria change the answer."""
    n_grid = 24
    for texture in ("vbars", "hbars", "mix"):
        I = _pair(texture, (0.3, 0.0))[0]
        gx, gy = R.scharr(I)
        exx, eyy = float((gx.astype(np.float64) ** 2).sum()), float((gy.astype(np.float64) ** 2).sum())
        ratio = exx / eyy
        assert (ratio > 20 if texture == "vbars" else ratio < 1 / 20 if texture == "hbars" else 0.5 < ratio < 2), (texture, ratio)
        for win in ROUTES:
            v = _oracle(texture, (0.49, -0.51), win, 0, 30, 0.001)[1]
            assert v[:n_grid].sum() >= n_grid // 2, (texture, win, v[:n_grid])
    for win in ROUTES:
        for only in ("vbars_only", "hbars_only"):
            assert not _oracle(only, (0.3, 0.0), win, 0, 30, 0.001)[1].any(), (only, win)
        v = _oracle("mix", (0.3, 0.0), win, 0, 30, 0.001)[1]
        assert v[n_grid:].any() and not v[n_grid:].all(), (win, v[n_grid:])
    p, v = _oracle("smooth", (6.0, 0.0), 51, 0, 30, 0.001)[:2]
    moved = np.abs(p - _tracks(51))[:n_grid][np.asarray(v[:n_grid], bool)]
    assert len(moved) >= n_grid // 2 and (moved[:, 0] > 4.0).all(), moved
    # a track that is alive after ONE Newton step and dead after two has a second origin outside the level: with a cap of three or thirty steps the
    # third iteration meets that origin in lk_outside INSIDE the loop (with a cap of two it is the final origin that ends it).  One per axis, both windows.
    for texture, shift, k in LEAVING:
        I, J = _pair(texture, shift)
        for win in ROUTES:
            pts = np.array(_tracks(win))
            st = {mc: KO.pyr_lk(I, J, pts, win=win, max_level=0, max_count=mc, eps=0.0)[1].ravel().astype(bool) for mc in (1, 2, 3, 30)}
            assert st[1][k] and not st[2][k] and not st[3][k] and not st[30][k], (texture, shift, win, [st[mc][k] for mc in st])
            other = 1 if shift[1] == 0.0 else 0  # the track's other coordinate is in the middle of the frame: one edge only
            assert abs(pts[k][other] - (H if other else W) / 2.0) < 1.0, pts[k]
    # the criteria matter: one step, three steps and thirty steps end at different positions, and so do eps 0.1 and eps 0
    for texture, shift in (("vbars", (0.49, -0.51)), ("hbars", (0.49, -0.51))):
        ends = {c: _oracle(texture, shift, 51, 0, *c)[0][:n_grid] for c in ((1, 0.0), (3, 0.0), (30, 0.0), (30, 0.1))}
        assert not np.array_equal(ends[(1, 0.0)], ends[(3, 0.0)]) and not np.array_equal(ends[(3, 0.0)], ends[(30, 0.0)])
        assert not np.array_equal(ends[(30, 0.0)], ends[(30, 0.1)])


@pytest.mark.gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("texture", TEXTURES)
def test_anisotropic_texture_under_every_criterion(texture, shift):
    _check_pair(texture, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("texture, shift", [c[:2] for c in LEAVING])
def test_tracks_that_leave_through_one_edge_during_the_iterations(texture, shift):
    _check_pair(texture, shift)


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [(6.0, 0.0), (0.0, -6.0), (6.0, -6.0)])
def test_six_pixel_shift_restages_the_search_region(shift):
    _check_pair("smooth", shift)


@pytest.mark.gpu
@pytest.mark.parametrize("scene", ["bars16", "bars16_neg"])
def test_largest_window_sums_of_both_signs(scene):
    """The grid tracks of lk_ref ('rand' offsets) are not used here: the track set is this file's, so the sums are those of its windows -- the scenes keep
    |Ix| = 4080 on every pixel of a column run, and the first Newton step's diff.Ix sum has one sign per scene."""
    def model(win, max_count, eps):
        I, J = R.SCENES[scene]()
        return R.lk_level0(I, J, _tracks(win), win, max_count, eps)

    _check_pair(scene, None, model=model)
